"""BatchNorm re-estimation on the device (cilrs_bn_train_stats, cilrs_net_forward_bn_stats,
cilrs_bn_stats_finalize; cilrs_mi355/bn_estimate.py; Trainer.update_bn), against the float64
definition of tests/_bn_estimate.py.

Budgets.  A table entry is a double chain over per-batch terms.  Against numpy float64 of the same
terms taken from the values the kernel read it may differ by
  * the chain's own rounding: (t + 2) * 2^-52 * sum|terms| (t additions and one or two roundings
    inside a term, all in double), and
  * the fp32 column reduce under the per-batch moment: the budget test_ops_edges_gpu.py already
    holds the BatchNorm statistics to inside the network's range of |mean|/std -- 1e-6 max(1, |mean|)
    for a mean, 1e-5 max(1, |var|) for an unbiased variance (there on the running buffers; applied
    here to the batch moment itself, which asks no less).  It enters row 0 / 1 once per batch, rows
    2 / 3 times M, row 3 as  d(var + mean^2) <= b_var (M-1)/M + 2 |mean| b_mean + b_mean^2.
The finalised buffers are one fp32 rounding (2^-24 |q|) away from the double quotient q of the
device's own table.

Plan level, seed-1 portable weights, batches of 3 / 5 / 2 frames at 40x120 (synthetic_batch seeds
10, 11, 12; the smallest layer then sees 16 rows): the gate on |d running_mean| / std and relative
|d running_var| against the float64 oracle is 10 x the same two figures of an fp32 CPU realisation,
measured in the test (torch's momentum=None procedure for "batch_mean"; the fp32 forward under the
definition for "pooled").

More than one data-parallel rank is not tested here (a world of one rank is).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _bn_estimate as E
import cilrs_oracle as O
from _guards import Inputs, all_finite, guarded

pytestmark = pytest.mark.gpu

H, W = 40, 120
SIZES_SEEDS = ((3, 10), (5, 11), (2, 12))
TOL_OUT = 1e-4                   # the project's output parity
B_MEAN, B_VAR = 1e-6, 1e-5       # test_ops_edges_gpu.py: rm / rv tolerances inside the network's range
U52, U24 = 2.0 ** -52, 2.0 ** -24
STATS_VARIANT = 1                # the architecture whose layers have 64, 512 and 2048 channels


def _L():
    from cilrs_mi355 import _lib as L
    return L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- op level ------------------------------------------------------------------------------------------
def _y(M, Cc, seed):
    """N(0,1) rows; every second channel moved to mean/std = 6 with a random sign (the off-zero case
    of test_ops_edges_gpu.py, R_NET_CEIL)"""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(Cc, generator=g) < 0.5, -1.0, 1.0)
    shift = 6.0 * sign * (torch.arange(Cc) % 2 == 1)
    return torch.randn(M, Cc, generator=g) + shift


class _Acc:
    """A guarded {t, sum M} | [4][C] table and exact partial scratch for cilrs_bn_train_stats."""

    def __init__(self, Cc):
        L = _L()
        self.C = Cc
        self.acc, self.check_acc = guarded(2 + 4 * Cc, torch.float64, 0.0, name="acc")
        self.part, self.check_part = guarded(L.lib().cilrs_bn_partial_floats(Cc), torch.float32,
                                             float("nan"), name="partial")

    def update(self, y):
        L = _L()
        yd = y.cuda()
        inp = Inputs(y=yd)
        rc = L.lib().cilrs_bn_train_stats(L.ptr(yd), y.size(0), self.C, L.ptr(self.acc),
                                          L.ptr(self.part), _stream())
        inp.check()
        self.check_acc()
        self.check_part()
        return rc

    def host(self):
        torch.cuda.synchronize()
        return self.acc.cpu().numpy().copy()


def _terms(ys):
    """per batch (M, mean, biased var, unbiased var) in numpy float64 from the fp32 values"""
    out = []
    for y in ys:
        y64 = y.double().numpy()
        M = y64.shape[0]
        mean = y64.mean(0)
        var = ((y64 - mean) ** 2).mean(0)
        out.append((M, mean, var, var * (M / (M - 1.0))))
    return out


def _check_table(acc, ys, what):
    """every entry of acc = {t, rows} | [4][C] inside the bound of the module docstring"""
    terms = _terms(ys)
    Cc, t = ys[0].size(1), len(ys)
    assert acc[0] == t and acc[1] == sum(M for M, *_ in terms)
    rows = acc[2:].reshape(4, Cc)
    ref, mag, fp32 = np.zeros((4, Cc)), np.zeros((4, Cc)), np.zeros((4, Cc))
    for M, mean, var, uvar in terms:
        bm = B_MEAN * np.maximum(1.0, np.abs(mean))
        bv = B_VAR * np.maximum(1.0, np.abs(uvar))
        for r, (term, bud) in enumerate((
                (mean, bm), (uvar, bv), (M * mean, M * bm),
                (M * (var + mean * mean), M * (bv * (M - 1.0) / M + 2 * np.abs(mean) * bm + bm * bm)))):
            ref[r] += term
            mag[r] += np.abs(term)
            fp32[r] += bud
    bound = (t + 2) * U52 * mag + fp32
    frac = np.abs(rows - ref) / bound
    print(f"BN-EST table {what}: worst |got - ref| / bound per row {frac.max(1)}; chain part of the "
          f"bound alone would allow {((t + 2) * U52 * mag / bound).max():.2e} of it")
    assert np.isfinite(rows).all() and frac.max() <= 1.0, (what, frac.max(1))


def _scatter(acc, Cc, variant=STATS_VARIANT):
    """a device table of `variant` whose first layer of C channels holds `acc` (device or numpy) and
    whose other layers hold one batch of 2 rows of zeros; returns (table, layer index)"""
    from cilrs_mi355.bn_estimate import stats_layout
    lay = stats_layout(variant)
    n = _L().lib().cilrs_variant_bn_stats_doubles(variant)
    table = torch.zeros(n, dtype=torch.float64)
    for _name, _c, head, _s in lay:
        table[head], table[head + 1] = 1.0, 2.0
    j = next(i for i, (_n, c, _h, _s) in enumerate(lay) if c == Cc)
    a = torch.as_tensor(np.asarray(acc.cpu() if torch.is_tensor(acc) else acc))
    table[lay[j][2]:lay[j][2] + 2] = a[:2]
    table[lay[j][3]:lay[j][3] + 4 * Cc] = a[2:]
    return table.cuda(), j


def _finalize(table, estimator, variant=STATS_VARIANT, expect_ok=True):
    """cilrs_bn_stats_finalize inside guard bands; ({layer: (rm, rv)} as CPU tensors, nbt) or the
    return code when a refusal is expected (then nothing may have been written)"""
    from cilrs_mi355.engine import _layout
    L = _L()
    lib = L.lib()
    bns = _layout(variant)[1]
    run, check_run = guarded(lib.cilrs_variant_bn_arena_floats(variant), torch.float32, float("nan"),
                             name="bn_running")
    nbt, check_nbt = guarded(len(bns), torch.int64, -7, name="bn_nbt")
    inp = Inputs(table=table) if table is not None else None
    rc = lib.cilrs_bn_stats_finalize(variant, L.ptr(table), estimator, L.ptr(run), L.ptr(nbt),
                                     _stream())
    check_run()
    check_nbt()
    if inp:
        inp.check()
    if not expect_ok:
        assert rc != 0
        assert bool(torch.isnan(run).all()) and bool((nbt == -7).all()), "a refused call wrote"
        return rc
    L.check(rc)
    all_finite(run, "bn_running")
    run, nbt = run.cpu(), nbt.cpu()
    return {j: (run[rm:rm + ch], run[rv:rv + ch]) for j, (_n, ch, rm, rv) in enumerate(bns)}, nbt


def _quotients(acc, Cc, estimator):
    """the double quotients of a {t, rows} | [4][C] table (numpy), and the scale of the pooled
    variance's cancellation"""
    t, N = acc[0], acc[1]
    r = acc[2:].reshape(4, Cc)
    if estimator == 0:
        return r[0] / t, r[1] / t, np.abs(r[1] / t)
    m = r[2] / N
    return m, (r[3] / N - m * m) * (N / (N - 1.0)), np.abs(r[3] / N) * (N / (N - 1.0))


@pytest.mark.parametrize("M", [2, 21, 3300])
@pytest.mark.parametrize("Cc", [64, 512, 2048])
def test_train_stats_table_and_finalize_against_float64(Cc, M):
    """two, then three updates of one table (the third batch has another row count), every entry
    inside the bound; then both estimators within one fp32 rounding of the double quotient of the
    device's own table"""
    M3 = max(2, M // 2 + 1)
    ys = [_y(M, Cc, 100 + Cc + M), _y(M, Cc, 200 + Cc + M), _y(M3, Cc, 300 + Cc + M)]
    a = _Acc(Cc)
    for y in ys[:2]:
        _L().check(a.update(y))
    _check_table(a.host(), ys[:2], f"C={Cc} M={M} two updates")
    _L().check(a.update(ys[2]))
    acc = a.host()
    _check_table(acc, ys, f"C={Cc} M={M},{M},{M3} three updates")
    table, j = _scatter(acc, Cc)
    for est in (0, 1):
        bufs, nbt = _finalize(table, est)
        assert int(nbt[j]) == 3 and bool((nbt == 1).sum() == nbt.numel() - 1)
        qm, qv, scale = _quotients(acc, Cc, est)
        rm, rv = bufs[j][0].double().numpy(), bufs[j][1].double().numpy()
        # one fp32 rounding of q; the double quotient itself is reproduced to a few units of 2^-52 of
        # the terms it subtracts
        em = np.abs(rm - qm) / (U24 * np.abs(qm) + 8 * U52 * np.abs(qm) + 2.0 ** -149)
        ev = np.abs(rv - qv) / (U24 * np.abs(qv) + 8 * U52 * scale + 2.0 ** -149)
        print(f"BN-EST finalize C={Cc} M={M} estimator {est}: |got - q| over one fp32 rounding "
              f"mean {em.max():.3f} var {ev.max():.3f}")
        assert em.max() <= 1.0 and ev.max() <= 1.0
        assert (rv >= 0).all()


@pytest.mark.parametrize("Cc,M", [(64, 21), (2048, 3300)])
def test_tables_add_and_runs_repeat_bit_for_bit(Cc, M):
    """table(A) + table(B) on the host IS the table that saw A then B (B one batch: its chain starts
    from zero, so the host's addition is the chain's next one); so are the finalised buffers, for
    both estimators; and a second run of everything is bit-identical"""
    ys = [_y(M, Cc, 1), _y(M - 1, Cc, 2), _y(M, Cc, 3)]

    def run(batches):
        a = _Acc(Cc)
        for y in batches:
            _L().check(a.update(y))
        torch.cuda.synchronize()
        return a.acc.clone()

    tab_a, tab_b, tab_ab, again = run(ys[:2]), run(ys[2:]), run(ys), run(ys)
    assert torch.equal(tab_ab, again), "two runs over the same batches differ"
    summed = (tab_a.cpu() + tab_b.cpu()).cuda()
    assert torch.equal(summed, tab_ab), "table(A) + table(B) != table(A then B)"
    for est in (0, 1):
        one, n1 = _finalize(_scatter(tab_ab, Cc)[0], est)
        two, n2 = _finalize(_scatter(summed, Cc)[0], est)
        assert torch.equal(n1, n2)
        assert all(torch.equal(one[j][0], two[j][0]) and torch.equal(one[j][1], two[j][1]) for j in one)


def test_op_level_refusals_launch_nothing():
    L = _L()
    lib = L.lib()
    Cc = 64
    a = _Acc(Cc)
    y = _y(8, Cc, 5).cuda()
    before = a.acc.clone()
    for rc in (lib.cilrs_bn_train_stats(L.ptr(y), 1, Cc, L.ptr(a.acc), L.ptr(a.part), _stream()),
               lib.cilrs_bn_train_stats(L.ptr(y), 8, Cc, None, L.ptr(a.part), _stream()),
               lib.cilrs_bn_train_stats(L.ptr(y), 8, Cc, L.ptr(a.acc[1:].view(torch.uint8)[4:]),
                                        L.ptr(a.part), _stream()),
               lib.cilrs_bn_train_stats(None, 8, Cc, L.ptr(a.acc), L.ptr(a.part), _stream())):
        assert rc != 0
    torch.cuda.synchronize()
    a.check_acc()
    a.check_part()
    assert torch.equal(a.acc, before) and bool(torch.isnan(a.part).all())
    # finalize: NULL table, a layer with t == 0, an unknown estimator
    n = lib.cilrs_variant_bn_stats_doubles(0)
    _finalize(None, 0, variant=0, expect_ok=False)
    _finalize(torch.zeros(n, dtype=torch.float64, device="cuda"), 0, variant=0, expect_ok=False)
    assert b"batch" in lib.cilrs_last_error()
    table, _j = _scatter(np.concatenate([[3.0, 24.0], np.ones(4 * 64)]), 64, variant=0)
    _finalize(table, 2, variant=0, expect_ok=False)
    one_empty = table.clone()
    one_empty[2 * 35] = 0.0                                   # the last layer alone saw nothing
    _finalize(one_empty, 1, variant=0, expect_ok=False)
    _finalize(table, 1, variant=0)                            # (the same table is served otherwise)


# ---- plan level ----------------------------------------------------------------------------------------
def _batches():
    return [O.synthetic_batch(b, seed=s, h=H, w=W) for b, s in SIZES_SEEDS]


def _dev(b):
    return tuple(t.cuda() for t in b[:4])


def _to64(b):
    return tuple(t.double() if t.is_floating_point() else t for t in b[:3])


def _model(seed=1):
    from cilrs_mi355 import CILRS
    m = CILRS(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), seed), strict=True)
    return m.cuda().eval()


def _buffers_of(m):
    """{layer name: (rm, rv, nbt)} of an engine-backed module, numpy float64"""
    torch.cuda.synchronize()
    return {n: (bn.running_mean.detach().cpu().double().numpy(),
                bn.running_var.detach().cpu().double().numpy(), int(bn.num_batches_tracked))
            for n, bn in E.bn_layers(m)}


@pytest.fixture(scope="module")
def world():
    """the float64 oracle's re-estimated buffers and the fp32 CPU realisations' (computed once)"""
    batches = _batches()
    orc64 = O.build_oracle(1).double()
    b64 = [_to64(b) for b in batches]
    orc32 = O.build_oracle(1)
    ref = {e: E.reestimate(orc64, b64, e) for e in ("batch_mean", "pooled")}
    cpu32 = {"batch_mean": E.torch_update_bn(orc32, batches),
             "pooled": E.reestimate(orc32, batches, "pooled")}
    floor = {e: E.buffer_errors(cpu32[e], ref[e]) for e in ref}
    return dict(batches=batches, orc64=orc64, ref=ref, floor=floor)


def _plan_stats(pl):
    """every convolution's mean | rstd | scale | shift from the plan's workspace (device clones) and
    the rows each BatchNorm sees"""
    L = _L()
    out, rows = [], []
    ws = pl.workspace.view(torch.float32)
    for ci in range(36):
        off, ch, M, j = L.sz(), L.i32(), L.i32(), L.i32()
        L.check(L.lib().cilrs_net_bn_layer_info(pl.handle, ci, C.byref(off), C.byref(ch), C.byref(M),
                                                C.byref(j)))
        out.append(ws[off.value:off.value + 4 * ch.value].clone())
        rows.append(M.value)
    return out, rows


def test_stats_forward_touches_no_buffer_and_is_the_train_forward(world):
    from cilrs_mi355.bn_estimate import BatchNormEstimator
    m = _model()
    eng = m.engine()
    est = BatchNormEstimator(m)
    least = 10 ** 9
    for b in world["batches"]:
        img, spd, cmd, _t = _dev(b)
        keep = (eng.bn.clone(), eng.nbt.clone(), eng.params.clone())
        est.update(img)
        torch.cuda.synchronize()
        assert torch.equal(eng.bn, keep[0]) and torch.equal(eng.nbt, keep[1])
        assert torch.equal(eng.params, keep[2])
        pl = eng.last_plan
        mine, rows = _plan_stats(pl)
        least = min(least, min(rows))
        # the tick-following entries refuse as after a train step
        with pytest.raises(RuntimeError, match="train mode"):
            eng.run_heads_mc(spd, cmd, 4, 0.5)
        eng.run_forward(img, spd, cmd, True, 0.0, 0)
        torch.cuda.synchronize()
        assert eng.last_plan is pl
        theirs, _ = _plan_stats(pl)
        bad = [ci for ci in range(36) if not torch.equal(mine[ci], theirs[ci])]
        assert not bad, f"per-layer statistics differ from cilrs_net_forward(train=1) on convs {bad}"
        with torch.no_grad():                                  # (the train forward moved them)
            eng.bn.copy_(keep[0])
            eng.nbt.copy_(keep[1])
    assert least == 16
    assert est.batches == 3
    head = est.table[:72].cpu().view(36, 2)
    assert bool((head[:, 0] == 3).all())
    assert float(head[0, 1]) == 10 * 20 * 60                   # the stem: 10 frames of 20 x 60 rows


@pytest.mark.parametrize("estimator", ["batch_mean", "pooled"])
def test_finalized_buffers_against_the_float64_oracle(world, estimator):
    """Measured on an MI355X (|d mean| / std, relative |d var|; fp32 CPU realisation beside it):
    see DESIGN.md section 5c."""
    from cilrs_mi355 import update_bn
    m = _model()
    update_bn(m, [_dev(b) for b in world["batches"]], estimator=estimator)
    got = _buffers_of(m)
    assert all(v[2] == 3 for v in got.values()) and len(got) == 36
    em, ev, where, vmin = E.buffer_errors(got, world["ref"][estimator])
    fm, fv, fwhere, _ = world["floor"][estimator]
    print(f"BN-EST plan {estimator}: HIP vs float64 oracle |d mean|/std {em:.3e} ({where}) rel |d var| "
          f"{ev:.3e}; fp32 CPU realisation {fm:.3e} ({fwhere}) {fv:.3e}; smallest running_var {vmin:.4f}")
    assert vmin > 0.01                                         # no degenerate channel in the gate
    assert em <= 10 * fm and ev <= 10 * fv


def test_eval_paths_pick_up_the_new_buffers(world):
    """Every eval realisation first runs on the OLD buffers (so whatever it caches is cached), then
    the buffers are re-estimated, then each must agree with the float64 oracle carrying ITS
    re-estimated buffers: model(...), the per-layer uint8 entry, the persistent single-frame launch
    (1e-4), and the fp16 trunk (test_infer16_gpu.py's end-to-end criterion: rms(HIP - emu64) on the
    pooled features <= 2 x rms(emu32 - emu64) of the CPU emulation of the same rounded computation)."""
    import copy
    import infer16_emulation as X
    from cilrs_mi355.bn_estimate import BatchNormEstimator
    from test_infer16_gpu import _PlanView
    m = _model()
    eng = m.engine()
    img, spd, cmd, _t, u8 = world["batches"][1]
    dimg, dspd, dcmd = img.cuda(), spd.cuda(), cmd.cuda()
    du8 = torch.from_numpy(u8).cuda()

    def run_all():
        with torch.no_grad():
            a = m(dimg, dspd, dcmd)
        b = eng.run_forward_u8(du8, dspd, dcmd)
        c = eng.run_forward_u8(du8[:1], dspd[:1], dcmd[:1], persistent=True)
        d = eng.run_forward_u8(du8, dspd, dcmd, half=True)
        torch.cuda.synchronize()
        feats = _PlanView(eng.last_plan, "fp16").io()[1]
        return [(x[0].cpu().double(), x[1].cpu().double()) for x in (a, b, c, d)], feats

    old, _ = run_all()
    est = BatchNormEstimator(m)
    for b in world["batches"]:
        est.update(b[0].cuda())
    est.finalize()
    new, feats = run_all()
    eng.check_status()

    orc = E.load_buffers(copy.deepcopy(world["orc64"]), world["ref"]["batch_mean"]).eval()
    with torch.no_grad():
        rc, rs = orc(img.double(), spd.double(), cmd)
        oc, _os = world["orc64"].eval()(img.double(), spd.double(), cmd)
    moved = float((rc - oc).abs().max())
    assert moved > 100 * TOL_OUT, "the re-estimated buffers do not move the outputs: no teeth"
    for name, (c, s), n in (("model(...)", new[0], 5), ("per-layer u8", new[1], 5),
                            ("persistent", new[2], 1)):
        err = max(float((c - rc[:n]).abs().max()), float((s - rs[:n]).abs().max()))
        print(f"BN-EST eval {name} with the new buffers vs float64 oracle: {err:.3e} "
              f"(old vs new buffers move the oracle's outputs by {moved:.3e})")
        assert err <= TOL_OUT
    assert float((old[0][0] - rc).abs().max()) > 100 * TOL_OUT
    # fp16 trunk: the emulation folds the fp32 module's buffers
    orc32 = E.load_buffers(O.build_oracle(1), world["ref"]["batch_mean"]).eval()
    e64 = X.features(orc32, img, torch.float16, torch.float64)
    e32 = X.features(orc32, img, torch.float16, torch.float32).double()
    rms = lambda d: float(d.pow(2).mean().sqrt())
    d_hip, d_cpu = feats.double() - e64, e32 - e64
    stale = rms(X.features(O.build_oracle(1).eval(), img, torch.float16, torch.float64) - e64)
    print(f"BN-EST eval fp16 trunk: rms(HIP - emu64) {rms(d_hip):.3e}, rms(emu32 - emu64) "
          f"{rms(d_cpu):.3e}; a fold of the old buffers would be {stale:.3e} away")
    assert stale > 20 * rms(d_cpu)
    assert rms(d_hip) <= 2.0 * rms(d_cpu)


def test_pooled_stem_does_not_depend_on_the_batching(world):
    """the 3-frame and the 2-frame batch against one batch of the same 5 frames: two estimates of the
    same moments, each inside the per-batch fp32 budget of the module docstring, plus the rounding to
    fp32"""
    from cilrs_mi355 import update_bn
    b2, b3 = world["batches"][0], world["batches"][2]
    one = torch.cat([b2[0], b3[0]]).cuda()
    ma, mb = _model(), _model()
    update_bn(ma, [b2[0].cuda(), b3[0].cuda()], estimator="pooled")
    update_bn(mb, [one], estimator="pooled")
    a, b = _buffers_of(ma)["visual_encoder.1"], _buffers_of(mb)["visual_encoder.1"]
    assert (a[2], b[2]) == (2, 1)
    bm = B_MEAN * np.maximum(1.0, np.abs(b[0]))
    bv = B_VAR * np.maximum(1.0, np.abs(b[1])) + 2 * np.abs(b[0]) * bm + bm * bm
    fm = np.abs(a[0] - b[0]) / (2 * bm + 2 * U24 * np.abs(b[0]))
    fv = np.abs(a[1] - b[1]) / (2 * bv * 1.001 + 2 * U24 * np.abs(b[1]))
    print(f"BN-EST pooled stem, 3 + 2 frames in two batches vs one: mean {np.abs(a[0] - b[0]).max():.3e} "
          f"var {np.abs(a[1] - b[1]).max():.3e}; as fractions of the bound {fm.max():.3f} {fv.max():.3f}")
    assert fm.max() <= 1.0 and fv.max() <= 1.0
    # a later layer does depend on it (its input was normalised per batch): the estimator is not
    # simply ignoring the batching
    la, lb = _buffers_of(ma)["visual_encoder.7.2.bn2"], _buffers_of(mb)["visual_encoder.7.2.bn2"]
    assert np.abs(la[1] - lb[1]).max() > 1e-4 * np.abs(lb[1]).max()


def test_resnet50_variant_once():
    import resnet50_oracle as R
    from cilrs_mi355 import CILRSResNet50, update_bn
    batches = [O.synthetic_batch(b, seed=s, h=88, w=200) for b, s in ((3, 10), (2, 11))]
    orc32 = R.build_oracle50(1)
    m = CILRSResNet50(4, 0.0)
    m.load_state_dict(orc32.state_dict(), strict=True)
    m = m.cuda().eval()
    ref = E.reestimate(R.build_oracle50(1).double(), [_to64(b) for b in batches])
    floor = E.buffer_errors(E.torch_update_bn(orc32, batches), ref)
    update_bn(m, [b[0].cuda() for b in batches])
    got = _buffers_of(m)
    assert len(got) == 53 and all(v[2] == 2 for v in got.values())
    em, ev, where, vmin = E.buffer_errors(got, ref)
    print(f"BN-EST plan ResNet-50 88x200: HIP vs float64 oracle |d mean|/std {em:.3e} ({where}) rel "
          f"|d var| {ev:.3e}; fp32 CPU realisation {floor[0]:.3e} {floor[1]:.3e}; smallest "
          f"running_var {vmin:.4f}")
    assert em <= 10 * floor[0] and ev <= 10 * floor[1]


def test_plan_level_refusals_launch_nothing():
    from cilrs_mi355.engine import PLAN_BF16_TRAIN, Plan
    L = _L()
    lib = L.lib()
    m = _model()
    eng = m.engine()
    n = lib.cilrs_variant_bn_stats_doubles(0)
    table, check_table = guarded(n, torch.float64, 0.0, name="table")

    def refused(pl, img, tab, word):
        bufs = L.Buffers(eng.params.data_ptr(), eng.grads.data_ptr(), eng.bn.data_ptr(),
                         eng.nbt.data_ptr(), pl.workspace.data_ptr())
        pl.workspace.fill_(0x5A)
        keep = (eng.bn.clone(), eng.nbt.clone())
        sn, sc, sh, sw = img.stride()
        rc = lib.cilrs_net_forward_bn_stats(pl.handle, C.byref(bufs), L.ptr(img), sn, sc, sh, sw,
                                            L.ptr(tab) if tab is not None else None, _stream())
        assert rc != 0 and word in lib.cilrs_last_error(), lib.cilrs_last_error()
        torch.cuda.synchronize()
        check_table()
        assert bool((pl.workspace == 0x5A).all()), "a refused call launched something"
        assert bool((table == 0).all())
        assert torch.equal(eng.bn, keep[0]) and torch.equal(eng.nbt, keep[1])

    img = torch.randn(2, 3, H, W, device="cuda")
    refused(Plan(eng.device, 2, H, W, 0, PLAN_BF16_TRAIN), img, table, b"fp32 plans only")
    pl = Plan(eng.device, 2, H, W, 0, 0)
    refused(pl, img, None, b"NULL")
    refused(pl, img, table.view(torch.uint8)[4:-4].view(torch.float32), b"aligned")
    # one frame of 32 x 32: layer4 is a 1 x 1 map, one value per channel
    refused(Plan(eng.device, 1, 32, 32, 0, 0), torch.randn(1, 3, 32, 32, device="cuda"), table,
            b"more than 1")
    # the Python front end refuses a bf16 engine before anything is built
    from cilrs_mi355.bn_estimate import BatchNormEstimator
    m2 = _model()
    m2.engine().train_precision = "bf16"
    with pytest.raises(RuntimeError, match="fp32 plans only"):
        BatchNormEstimator(m2)
    with pytest.raises(RuntimeError, match="no batch"):
        BatchNormEstimator(m).finalize()


# ---- Trainer ---------------------------------------------------------------------------------------------
def _ema_trainer(steps=2, process_group=None):
    import dataclasses
    from cilrs_mi355 import CONFIG_A, Trainer
    m = _model()
    tr = Trainer(m, dataclasses.replace(CONFIG_A, ema_decay=0.9), process_group=process_group)
    for s in range(steps):
        tr.train_step(*_dev(O.synthetic_batch(4, seed=40 + s, h=H, w=W)))
    m.eval()
    return m, tr


def test_update_bn_of_the_averaged_weights(world):
    from cilrs_mi355 import CONFIG_A, Trainer, update_bn
    m, tr = _ema_trainer()
    eng = tr.eng
    batches = [_dev(b) for b in world["batches"]]
    val = [_dev(O.synthetic_batch(4, seed=77, h=H, w=W))]
    torch.cuda.synchronize()
    live = (eng.bn.clone(), eng.nbt.clone(), eng.params.clone())
    # before any update_bn(ema=True): the averaged weights run on the live buffers
    assert tr.ema_bn is None and tr.ema_bn_state_dict() is None
    with tr.ema_weights():
        assert torch.equal(eng.bn, live[0]) and torch.equal(eng.nbt, live[1])
        assert not torch.equal(eng.params, live[2])
    tr.update_bn(batches, ema=True)
    torch.cuda.synchronize()
    assert torch.equal(eng.bn, live[0]) and torch.equal(eng.nbt, live[1])
    assert torch.equal(eng.params, live[2])
    # an independent module with the averaged parameters and the live buffers, re-estimated
    m2 = _model()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    sd.update(tr.ema_state_dict())
    m2.load_state_dict(sd, strict=True)
    update_bn(m2, batches)
    want = {k: v.detach().cpu() for k, v in m2.state_dict().items()}
    ema_bn = tr.ema_bn_state_dict()
    assert len(ema_bn) == 3 * 36
    assert all(torch.equal(v, want[k]) for k, v in ema_bn.items())
    assert int(ema_bn["visual_encoder.1.num_batches_tracked"]) == 3
    img, spd, cmd, _t = val[0]
    with tr.ema_weights():
        inside = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        with torch.no_grad():
            c1, s1 = m(img, spd, cmd)
        assert all(torch.equal(v, tr.ema_bn_state_dict()[k]) for k, v in ema_bn.items())
    assert all(torch.equal(inside[k], want[k]) for k in want)
    with torch.no_grad():
        c2, s2 = m2(img, spd, cmd)
    assert torch.equal(c1, c2) and torch.equal(s1, s2)
    def flat(res):                       # (a command without a sample reports NaN: compare as text)
        return [(k, repr(v)) for d in res for k, v in sorted(d.items())]

    assert flat(tr.validate(val, ema=True)) == flat(Trainer(m2, CONFIG_A).validate(val))
    assert flat(tr.validate(val, ema=True)) != flat(tr.validate(val))
    torch.cuda.synchronize()
    assert torch.equal(eng.bn, live[0]) and torch.equal(eng.params, live[2])
    # ema=False is the plain update_bn of the live weights
    m3 = _model()
    m3.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, strict=True)
    update_bn(m3, batches, estimator="pooled")
    tr.update_bn(batches, estimator="pooled")
    assert all(torch.equal(v.cpu(), m3.state_dict()[k].cpu()) for k, v in m.state_dict().items())
    with tr.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.update_bn(batches)


LATEST_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict",
               "loop_state", "ema_state_dict", "ema_updates"}
BEST_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "val_loss", "val_steer", "config",
             "cmd_steer_errors", "ema"}


def test_fit_checkpoints_the_averaged_weights_buffers(world, tmp_path):
    from cilrs_mi355 import checkpoint
    from cilrs_mi355.loop import fit
    train = lambda: [_dev(O.synthetic_batch(4, seed=50, h=H, w=W))]
    val = lambda: [_dev(O.synthetic_batch(4, seed=77, h=H, w=W))]
    bn_batches = lambda: [b[0].cuda() for b in world["batches"][:2]]
    # without ema_bn_batches: today's keys
    m0, tr0 = _ema_trainer(steps=0)
    d0 = str(tmp_path / "plain")
    fit(tr0, train, val, epochs=1, out_dir=d0, log=lambda *_: None)
    latest0 = checkpoint.load_file(os.path.join(d0, "checkpoint_latest.pth"))
    best0 = checkpoint.load_file(os.path.join(d0, "checkpoint_best.pth"))
    assert set(latest0) == LATEST_KEYS and set(best0) == BEST_KEYS
    assert set(best0["ema"]) == {"decay", "updates"}
    assert torch.equal(best0["model_state_dict"]["visual_encoder.1.running_mean"],
                       m0.state_dict()["visual_encoder.1.running_mean"].cpu())
    # with it
    m1, tr1 = _ema_trainer(steps=0)
    d1 = str(tmp_path / "bn")
    fit(tr1, train, val, epochs=1, out_dir=d1, log=lambda *_: None, ema_bn_batches=bn_batches)
    latest1 = checkpoint.load_file(os.path.join(d1, "checkpoint_latest.pth"))
    best1 = checkpoint.load_file(os.path.join(d1, "checkpoint_best.pth"))
    assert set(latest1) == LATEST_KEYS | {"ema_bn_state_dict"} and set(best1) == BEST_KEYS
    assert best1["ema"]["bn"] is True
    ema_bn = tr1.ema_bn_state_dict()
    assert set(latest1["ema_bn_state_dict"]) == set(ema_bn)
    assert all(torch.equal(v, ema_bn[k]) for k, v in latest1["ema_bn_state_dict"].items())
    assert all(torch.equal(best1["model_state_dict"][k], v) for k, v in ema_bn.items())
    assert int(ema_bn["visual_encoder.1.num_batches_tracked"]) == 2
    # the live buffers in the latest file are the live model's, not the re-estimated ones
    assert torch.equal(latest1["model_state_dict"]["visual_encoder.1.running_mean"],
                       m1.state_dict()["visual_encoder.1.running_mean"].cpu())
    assert not torch.equal(latest1["model_state_dict"]["visual_encoder.1.running_mean"],
                           ema_bn["visual_encoder.1.running_mean"])
    # resume restores the pair bit for bit
    m2, tr2 = _ema_trainer(steps=0)
    checkpoint.load(os.path.join(d1, "checkpoint_latest.pth"), m2, tr2)
    torch.cuda.synchronize()
    assert torch.equal(tr2.ema_bn, tr1.ema_bn) and torch.equal(tr2.ema_nbt, tr1.ema_nbt)
    assert torch.equal(tr2.ema, tr1.ema)


def test_world_of_one_rank_all_reduces_the_table_to_itself(world, tmp_path):
    import torch.distributed as dist
    from cilrs_mi355 import CONFIG_A, Trainer, update_bn
    batches = [_dev(b) for b in world["batches"]]
    alone = _model()
    est0 = update_bn(alone, batches)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        m = _model()
        tr = Trainer(m, CONFIG_A, process_group=dist.group.WORLD)
        est = tr.update_bn(batches)
        torch.cuda.synchronize()
        assert torch.equal(est.table, est0.table)
        assert all(torch.equal(v, alone.state_dict()[k]) for k, v in m.state_dict().items())
    finally:
        dist.destroy_process_group()
