"""Feature-space novelty on the device (csrc/novelty.hip: cilrs_feature_moments,
cilrs_feature_novelty, their plan-level forms, cilrs_mi355.novelty.FeatureDensity and
Predictor.predict_novelty) against the float64 definition of tests/_novelty.py.

Gates.  Moment table: every entry within rows * 2^-52 * sum_b |x_bi x_bj| of numpy float64 (one fma
chain of `rows` steps errs by at most rows * 2^-53 of that sum to first order, numpy's own sum by as
much); the counts are exact.  Score: d2 against the float64 evaluation of THE SAME rounded fp32
tables, within
    e_i = (i + 18) 2^-24 sum_j |W_ij||u_j|                     per row (i + 1 products, their sums
                                                               and the six butterfly steps),
    sum_i (2 |y_i| e_i + e_i^2) + (F + 16) 2^-24 sum_i y_i^2   for the sum of squares
(tests/_novelty.py, score).  Outputs are NaN-pre-filled inside guard bands (tests/_guards.py), the
scratch is exactly sized, the columns j > i of W hold NaN on the device: they must not be read.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import _guards as G
import _novelty as N
import cilrs_oracle as O
import test_mc_dropout_gpu as TM

pytestmark = pytest.mark.gpu

_CACHE = {}


def _lib():
    from cilrs_mi355 import _lib as L
    return L


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err():
    msg = _lib().lib().cilrs_last_error()
    return msg.decode() if msg else ""


def _commands(rows, NC, seed, absent=True, bad=True):
    """commands 0..NC-1 with the last one absent; one row out of range when there are rows to spare"""
    rng = np.random.default_rng(seed)
    top = NC - 1 if absent and NC > 1 else NC
    cmd = rng.integers(0, top, size=rows).astype(np.int64)
    if rows >= 3:
        cmd[:top] = np.arange(top)[:rows]
    if bad and rows >= 5:
        cmd[rows // 2] = NC + 3
    return cmd


def _source(kind, rows, F, NC, ld, hw, seed):
    """(v fp32 [rows][F] as the device takes it, features_d / ld, featmap_d / hw)"""
    if kind == "pooled":
        v, _ = N.relu_features(rows, F, NC, seed)
        return v, TM._pooled_dev(torch.from_numpy(v), ld), ld, None, 0
    fm, _ = N.relu_features(rows * hw, F, NC, seed)
    fm = fm.reshape(rows, hw, F)
    return N.pool_cell_order(fm), None, 0, torch.from_numpy(fm).cuda(), hw


SENTINEL = 7.0          # what the never-defined entries j > i of G hold before and after a call


def _new_table(F, NC):
    L = _lib()
    n = L.lib().cilrs_feature_moments_doubles(F, NC)
    assert n == N.table_doubles(F, NC)
    t, check = G.guarded(n, dtype=torch.float64, fill=0.0, name="table")
    Gv = t[NC * (F + 1):].view(F, F)
    Gv += torch.triu(torch.full((F, F), SENTINEL, dtype=torch.float64, device="cuda"), 1)
    return t, check


def _moments(feat_d, ld, fm_d, hw, cmd_d, rows, F, NC, piv_d, table, status):
    L = _lib()
    L.check(L.lib().cilrs_feature_moments(L.ptr(feat_d), ld, L.ptr(fm_d), hw, L.ptr(cmd_d), rows, F, NC,
                                          L.ptr(piv_d), L.ptr(table), L.ptr(status), _st()))


def _check_table(table, v, cmd, piv, F, NC, what, rows_total=None):
    n, s, Gd = N.split(table.cpu().numpy(), F, NC)
    nr, sr, Gr = N.split(N.moments(v, cmd, piv, NC), F, NC)
    bG, bx = N.moments_bound(v, piv, rows_total)
    assert np.array_equal(n, nr), (what, n, nr)
    k = N.branch(cmd, NC)
    bs = np.stack([bx[k == c].sum(axis=0) for c in range(NC)])
    es, eG = np.abs(s - sr), np.abs(np.tril(Gd) - np.tril(Gr))
    share = max(float((eG / np.maximum(bG, 1e-300))[np.tril(np.ones((F, F), bool))].max()),
                float((es / np.maximum(bs, 1e-300)).max()))
    print(f"moments {what}: largest share of the bound {share:.3g} (G max err {eG.max():.3g}, "
          f"s max err {es.max():.3g})")
    assert (eG <= bG).all() and (es <= bs).all(), what
    up = np.triu(np.ones((F, F), bool), 1)
    assert (Gd[up] == SENTINEL).all(), f"{what}: entries j > i of G were written"


# ---- moments, op level -----------------------------------------------------------------------------
MOMENT_CASES = {
    # name: (F, rows, ld - F, NC, source, hw)
    "f512_r1_nc2": (512, 1, 0, 2, "pooled", 0),
    "f512_r5_ld_nc4": (512, 5, 128, 4, "pooled", 0),
    "f512_r37_nc6_map6": (512, 37, 0, 6, "map", 6),
    "f512_r37_ld_nc4": (512, 37, 128, 4, "pooled", 0),
    "f512_r5_nc4_map21": (512, 5, 0, 4, "map", 21),
    "f2048_r1_ld_nc6": (2048, 1, 128, 6, "pooled", 0),
    "f2048_r5_nc2_map21": (2048, 5, 0, 2, "map", 21),
    "f2048_r37_ld_nc4": (2048, 37, 128, 4, "pooled", 0),
}


@pytest.mark.parametrize("case", list(MOMENT_CASES))
def test_moments_op_level_against_float64(case):
    F, rows, pad, NC, kind, hw = MOMENT_CASES[case]
    seed = list(MOMENT_CASES).index(case) + 11
    v, feat_d, ld, fm_d, hw = _source(kind, rows, F, NC, F + pad, hw, seed)
    cmd = _commands(rows, NC, seed)
    piv = (v.mean(axis=0) + 0.05 * np.random.default_rng(seed).standard_normal(F)).astype(np.float32)
    cmd_d, piv_d = torch.from_numpy(cmd).cuda(), torch.from_numpy(piv).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    table, check = _new_table(F, NC)
    ins = G.Inputs(features=feat_d, featmap=fm_d, command=cmd_d, pivot=piv_d)
    _moments(feat_d, ld, fm_d, hw, cmd_d, rows, F, NC, piv_d, table, status)
    check()
    ins.check()
    _check_table(table, v, cmd, piv, F, NC, case)
    out_of_range = bool(((cmd < 0) | (cmd >= NC)).any())
    assert int(status.item()) == int(out_of_range)
    n = table[:NC].cpu().numpy()
    if NC > 1:
        assert n[NC - 1] == 0.0 and not table[NC + (NC - 1) * F:NC + NC * F].any()    # the absent command
    assert n.sum() == rows
    # two runs are bit-identical
    table2, check2 = _new_table(F, NC)
    _moments(feat_d, ld, fm_d, hw, cmd_d, rows, F, NC, piv_d, table2, None)
    check2()
    assert torch.equal(table2, table)


@pytest.mark.parametrize("F,kind", [(512, "pooled"), (512, "map"), (2048, "pooled")])
def test_moments_updates_of_2_plus_3_rows_equal_one_of_5(F, kind):
    NC, hw = 4, 6
    v, feat_d, ld, fm_d, hw = _source(kind, 5, F, NC, F + 128, hw, 3)
    cmd = np.array([2, 0, 1, 0, 2], dtype=np.int64)
    piv = v.mean(axis=0).astype(np.float32)
    cmd_d, piv_d = torch.from_numpy(cmd).cuda(), torch.from_numpy(piv).cuda()
    one, c1 = _new_table(F, NC)
    _moments(feat_d, ld, fm_d, hw, cmd_d, 5, F, NC, piv_d, one, None)
    two, c2 = _new_table(F, NC)
    part = lambda t, a, b: None if t is None else t[a:b]
    _moments(part(feat_d, 0, 2), ld, part(fm_d, 0, 2), hw, cmd_d[:2], 2, F, NC, piv_d, two, None)
    _moments(part(feat_d, 2, 5), ld, part(fm_d, 2, 5), hw, cmd_d[2:], 3, F, NC, piv_d, two, None)
    c1()
    c2()
    assert torch.equal(one, two)
    _check_table(two, v, cmd, piv, F, NC, f"2 + 3 rows F={F} {kind}", rows_total=5)
    # 37 + 5 rows: the second update continues chains that crossed the 32-row staging pass
    v2, f2, ld2, _fm, _hw = _source("pooled", 42, F, NC, F, 0, 4)
    cmd2 = _commands(42, NC, 4, bad=False)
    c2_d = torch.from_numpy(cmd2).cuda()
    a, ca = _new_table(F, NC)
    _moments(f2, ld2, None, 0, c2_d, 42, F, NC, piv_d, a, None)
    b, cb = _new_table(F, NC)
    _moments(f2[:37], ld2, None, 0, c2_d[:37], 37, F, NC, piv_d, b, None)
    _moments(f2[37:], ld2, None, 0, c2_d[37:], 5, F, NC, piv_d, b, None)
    ca()
    cb()
    assert torch.equal(a, b)
    _check_table(a, v2, cmd2, piv, F, NC, f"37 + 5 rows F={F}", rows_total=42)


# ---- score, op level ---------------------------------------------------------------------------------
def _tables(F, NC):
    """(mean32, W32) of a tests/_novelty.py fit of relu-shaped synthetic features with exactly-zero
    channels, and the device copies; the device W holds NaN in its columns j > i"""
    key = ("tables", F, NC)
    if key not in _CACHE:
        rows = 240
        v, cmd = N.relu_features(rows, F, NC, 100 + NC)
        cmd[cmd == NC - 1] = 0                             # the last command never occurs
        assert (v.max(axis=0) == 0.0).any()
        piv = v[:32].mean(axis=0).astype(np.float32)
        fin = N.finalize(N.moments(v, cmd, piv, NC), piv, F, NC, 0.01)
        Wd = torch.from_numpy(fin["W32"]).clone()
        Wd[torch.triu(torch.ones(F, F, dtype=torch.bool), 1)] = float("nan")
        _CACHE[key] = (fin["mean32"], fin["W32"], torch.from_numpy(fin["mean32"]).cuda(), Wd.cuda())
    return _CACHE[key]


class _ScoreOut:
    """guarded, NaN-filled d2 and an exactly sized, NaN-filled scratch"""

    def __init__(self, F, B, short=0):
        self.n = _lib().lib().cilrs_feature_novelty_scratch_floats(F, B)
        self.d2, c1 = G.guarded(B, name="d2")
        self.scratch, c2 = G.guarded(max(self.n - short, 1), name="scratch")
        self.checks = (c1, c2)

    def check(self):
        for c in self.checks:
            c()

    def untouched(self):
        self.check()
        assert bool(torch.isnan(self.d2).all()) and bool(torch.isnan(self.scratch).all()), \
            "a refused call wrote to its outputs"


def _score(feat_d, ld, fm_d, hw, cmd_d, B, F, NC, mean_d, W_d, status=None):
    L = _lib()
    out = _ScoreOut(F, B)
    ins = G.Inputs(features=feat_d, featmap=fm_d, command=cmd_d, mean=mean_d)
    L.check(L.lib().cilrs_feature_novelty(L.ptr(feat_d), ld, L.ptr(fm_d), hw, L.ptr(cmd_d), B, F, NC,
                                          L.ptr(mean_d), L.ptr(W_d), L.ptr(out.d2), L.ptr(out.scratch),
                                          out.n, L.ptr(status), _st()))
    out.check()
    ins.check()
    G.all_finite(out.d2, "d2")
    return out.d2.cpu()


def _check_d2(d2, v, cmd, mean32, W32, what):
    ref, bound = N.score(v, cmd, mean32, W32)
    err = np.abs(d2.double().numpy() - ref)
    share = float((err / bound).max())
    print(f"novelty {what}: largest share of the bound {share:.3g} (max rel err "
          f"{float((err / ref).max()):.3g}, d2 {ref.min():.4g} .. {ref.max():.4g})")
    assert (err <= bound).all(), (what, err, bound)


SCORE_CASES = {
    # name: (F, B, ld - F, NC, source, hw)
    "f512_b1_nc2": (512, 1, 0, 2, "pooled", 0),
    "f512_b3_nc4_map6": (512, 3, 0, 4, "map", 6),
    "f512_b5_ld_nc6": (512, 5, 128, 6, "pooled", 0),
    "f512_b33_nc4": (512, 33, 0, 4, "pooled", 0),
    "f2048_b1_nc4": (2048, 1, 0, 4, "pooled", 0),
    "f2048_b3_ld_nc6": (2048, 3, 128, 6, "pooled", 0),
    "f2048_b5_nc4_map21": (2048, 5, 0, 4, "map", 21),
    "f2048_b33_ld_nc4": (2048, 33, 128, 4, "pooled", 0),
}


@pytest.mark.parametrize("case", list(SCORE_CASES))
def test_score_op_level_against_float64(case):
    F, B, pad, NC, kind, hw = SCORE_CASES[case]
    seed = list(SCORE_CASES).index(case) + 31
    mean32, W32, mean_d, W_d = _tables(F, NC)
    v, feat_d, ld, fm_d, hw = _source(kind, B, F, NC, F + pad, hw, seed)
    cmd = _commands(B, NC, seed)                            # (its out-of-range row scores against mean 0)
    cmd_d = torch.from_numpy(cmd).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d2 = _score(feat_d, ld, fm_d, hw, cmd_d, B, F, NC, mean_d, W_d, status)
    _check_d2(d2, v, cmd, mean32, W32, case)
    assert int(status.item()) == int(bool(((cmd < 0) | (cmd >= NC)).any()))
    # two runs are bit-identical; frame b of a batch is the frame alone
    assert torch.equal(_score(feat_d, ld, fm_d, hw, cmd_d, B, F, NC, mean_d, W_d), d2)
    for b in sorted({0, B // 2, B - 1}):
        alone = _score(None if feat_d is None else feat_d[b:b + 1], ld,
                       None if fm_d is None else fm_d[b:b + 1], hw, cmd_d[b:b + 1], 1, F, NC, mean_d, W_d)
        assert torch.equal(alone[0], d2[b]), (case, b)


# ---- refusals ----------------------------------------------------------------------------------------
def _refusal_args():
    F, NC, B = 512, 4, 3
    v, feat_d, ld, _fm, _hw = _source("pooled", B, F, NC, F, 0, 7)
    fm = torch.zeros(B, 6, F, device="cuda")
    _m, _w, mean_d, W_d = _tables(F, NC)
    return dict(features=feat_d, ld=ld, featmap=None, hw=0, command=torch.tensor([1, 0, 2]).cuda(),
                B=B, F=F, NC=NC, pivot=torch.zeros(F, device="cuda"), mean=mean_d, W=W_d, fm=fm)


COMMON_REFUSALS = {
    "neither source": (dict(features=None), "exactly one"),
    "both sources": (dict(featmap="fm", hw=6), "exactly one"),
    "null command": (dict(command=None), "NULL"),
    "batch 0": (dict(B=0), "batch"),
    "batch negative": (dict(B=-2), "batch"),
    "F 500": (dict(F=500), "feature width"),
    "F 1024": (dict(F=1024), "feature width"),
    "NC 0": (dict(NC=0), "commands"),
    "NC 9": (dict(NC=9), "commands"),
    "ld below F": (dict(ld=511), "ld"),
    "map of 0 cells": (dict(features=None, featmap="fm", hw=0), "cells"),
}
MOMENT_REFUSALS = dict(COMMON_REFUSALS, **{
    "null pivot": (dict(pivot=None), "NULL"),
    "null table": (dict(null="table"), "NULL"),
})
SCORE_REFUSALS = dict(COMMON_REFUSALS, **{
    "null mean": (dict(mean=None), "NULL"),
    "null W": (dict(W=None), "NULL"),
    "null d2": (dict(null="d2"), "NULL"),
    "null scratch": (dict(null="scratch"), "scratch"),
    "scratch one float short": (dict(short=1), "scratch"),
})


@pytest.mark.parametrize("case", list(MOMENT_REFUSALS))
def test_moments_refusals_launch_nothing(case):
    change, text = MOMENT_REFUSALS[case]
    a = _refusal_args()
    change = dict(change)
    null = change.pop("null", None)
    a.update(change)
    if a["featmap"] == "fm":
        a["featmap"] = a["fm"]
    L = _lib()
    table, check = G.guarded(N.table_doubles(512, 4), dtype=torch.float64, name="table")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = L.lib().cilrs_feature_moments(L.ptr(a["features"]), a["ld"], L.ptr(a["featmap"]), a["hw"],
                                       L.ptr(a["command"]), a["B"], a["F"], a["NC"], L.ptr(a["pivot"]),
                                       None if null == "table" else L.ptr(table), L.ptr(status), _st())
    msg = _err()
    assert rc != 0, case
    assert text in msg, (case, msg)
    check()
    assert bool(torch.isnan(table).all()) and int(status.item()) == 0


@pytest.mark.parametrize("case", list(SCORE_REFUSALS))
def test_score_refusals_launch_nothing(case):
    change, text = SCORE_REFUSALS[case]
    a = _refusal_args()
    change = dict(change)
    null, short = change.pop("null", None), change.pop("short", 0)
    a.update(change)
    if a["featmap"] == "fm":
        a["featmap"] = a["fm"]
    L = _lib()
    out = _ScoreOut(512, 3, short=short)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = L.lib().cilrs_feature_novelty(
        L.ptr(a["features"]), a["ld"], L.ptr(a["featmap"]), a["hw"], L.ptr(a["command"]), a["B"],
        a["F"], a["NC"], L.ptr(a["mean"]), L.ptr(a["W"]), None if null == "d2" else L.ptr(out.d2),
        None if null == "scratch" else L.ptr(out.scratch), out.n - short, L.ptr(status), _st())
    msg = _err()
    assert rc != 0, case
    assert text in msg, (case, msg)
    out.untouched()
    assert int(status.item()) == 0


def test_size_queries():
    lib = _lib().lib()
    assert lib.cilrs_feature_moments_doubles(512, 4) == 4 * 513 + 512 * 512
    assert lib.cilrs_feature_moments_doubles(2048, 8) == 8 * 2049 + 2048 * 2048
    for F, NC in ((500, 4), (512, 0), (512, 9), (0, 4)):
        assert lib.cilrs_feature_moments_doubles(F, NC) == 0
    assert lib.cilrs_feature_novelty_scratch_floats(512, 3) >= 3 * 512
    for F, B in ((500, 3), (512, 0), (512, -1), (2048, 65537)):
        assert lib.cilrs_feature_novelty_scratch_floats(F, B) == 0


# ---- plan level --------------------------------------------------------------------------------------
PLAN_CASES = dict(TM.REALISATIONS)
PLAN_CASES["resnet50"] = (1, 40, 120, TM._fwd_per_layer, "combined")


def _plan_features32(pl, persistent):
    """fp32 pooled features exactly as the plan-level entries take them: `combined`, or after the
    persistent launch the cell-order average of the stored last feature map"""
    if persistent:
        fm = TM._plan_view(pl).fetch(35)                   # [B][C][HW]
        return N.pool_cell_order(fm.permute(0, 2, 1).contiguous().numpy())
    L = _lib()
    co, ld, feat = L.sz(), L.i32(), L.i32()
    L.check(L.lib().cilrs_net_infer16_io_info(pl.handle, None, None, C.byref(co), C.byref(ld),
                                              C.byref(feat)))
    comb = pl.workspace[co.value:co.value + 4 * pl.batch * ld.value].view(torch.float32)
    return comb.view(pl.batch, ld.value)[:, :feat.value].cpu().numpy().copy()


def _net_moments(pl, cmd_d, piv_d, table):
    L = _lib()
    return L.lib().cilrs_net_feature_moments(pl.handle, C.byref(pl.bufs), L.ptr(cmd_d), L.ptr(piv_d),
                                             L.ptr(table), _st())


def _net_novelty(pl, cmd_d, mean_d, W_d, out):
    L = _lib()
    return L.lib().cilrs_net_novelty(pl.handle, C.byref(pl.bufs), L.ptr(cmd_d), L.ptr(mean_d),
                                     L.ptr(W_d), L.ptr(out.d2), L.ptr(out.scratch), out.n, _st())


@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_plan_level_after_each_eval_realisation(name):
    B, H, W, fwd, _source_name = PLAN_CASES[name]
    m, _orc = TM._models50() if name == "resnet50" else TM._pair()
    F, NC = (2048, 4) if name == "resnet50" else (512, 4)
    eng = m.engine()
    _img, spd, cmd, _t, u8 = O.synthetic_batch(B, seed=77, h=H, w=W)
    u8_d, spd_d, cmd_d = torch.from_numpy(u8).cuda(), spd.cuda(), cmd.cuda()
    ctrl, ps = fwd(eng, u8_d, spd_d, cmd_d)
    torch.cuda.synchronize()
    pl = eng.last_plan
    eng.check_status()
    before = (ctrl.clone(), ps.clone())
    v = _plan_features32(pl, name == "persistent")
    assert v.shape == (B, F) and np.isfinite(v).all()
    what = f"plan {name} ({B},{H},{W})"
    L = _lib()
    # moments
    piv = (v.mean(axis=0) * 0.9).astype(np.float32)
    piv_d = torch.from_numpy(piv).cuda()
    table, check = _new_table(F, NC)
    L.check(_net_moments(pl, cmd_d, piv_d, table))
    check()
    _check_table(table, v, cmd.numpy(), piv, F, NC, what)
    # score (any lower-triangular W and means will do for the comparison: the op-level fit's)
    mean32, W32, mean_d, W_d = _tables(F, NC)
    out = _ScoreOut(F, B)
    L.check(_net_novelty(pl, cmd_d, mean_d, W_d, out))
    out.check()
    G.all_finite(out.d2, "d2")
    _check_d2(out.d2.cpu(), v, cmd.numpy(), mean32, W32, what)
    assert pl.status.tolist()[0] == 0
    # the forward's own outputs: untouched, and the same from the next forward
    assert torch.equal(ctrl, before[0]) and torch.equal(ps, before[1])
    ctrl2, ps2 = fwd(eng, u8_d, spd_d, cmd_d)
    torch.cuda.synchronize()
    assert torch.equal(ctrl2, before[0]) and torch.equal(ps2, before[1])
    # a command of 7: status word 0, command 0
    bad = cmd.clone()
    bad[0] = 7
    out2 = _ScoreOut(F, B)
    L.check(_net_novelty(pl, bad.cuda(), mean_d, W_d, out2))
    out2.check()
    assert pl.status.tolist()[0] == 1
    pl.status.zero_()
    torch.cuda.synchronize()
    _check_d2(out2.d2.cpu(), v, bad.numpy(), mean32, W32, what + " command 7")
    table2, check2 = _new_table(F, NC)
    L.check(_net_moments(pl, bad.cuda(), piv_d, table2))
    check2()
    assert pl.status.tolist()[0] == 1
    pl.status.zero_()
    torch.cuda.synchronize()
    _check_table(table2, v, bad.numpy(), piv, F, NC, what + " command 7")


def test_plan_level_refusals():
    m = TM._train_model()
    eng = m.engine()
    B, H, W, F, NC = 3, 40, 120, 512, 4
    img, spd, cmd, _t, _u8 = O.synthetic_batch(B, seed=5, h=H, w=W)
    spd_d, cmd_d = spd.cuda(), cmd.cuda()
    _m, _w, mean_d, W_d = _tables(F, NC)
    piv_d = torch.zeros(F, device="cuda")

    def both_refused(pl, text):
        table, check = G.guarded(N.table_doubles(F, NC), dtype=torch.float64, name="table")
        rc = _net_moments(pl, cmd_d, piv_d, table)
        assert rc != 0 and text in _err(), _err()
        check()
        assert bool(torch.isnan(table).all())
        out = _ScoreOut(F, B)
        rc = _net_novelty(pl, cmd_d, mean_d, W_d, out)
        assert rc != 0 and text in _err(), _err()
        out.untouched()

    both_refused(eng.plan(B, H, W, lane=3), "no forward")        # a plan no forward has run on
    _c, _s, pl = eng.run_forward(img.cuda(), spd_d, cmd_d, True, 0.5, 1)
    torch.cuda.synchronize()
    both_refused(pl, "train mode")
    eng.run_forward(img.cuda(), spd_d, cmd_d, False, 0.0, 0)
    torch.cuda.synchronize()
    L = _lib()
    out = _ScoreOut(F, B, short=1)
    rc = L.lib().cilrs_net_novelty(pl.handle, C.byref(pl.bufs), L.ptr(cmd_d), L.ptr(mean_d), L.ptr(W_d),
                                   L.ptr(out.d2), L.ptr(out.scratch), out.n - 1, _st())
    assert rc != 0 and "scratch" in _err()
    out.untouched()
    out = _ScoreOut(F, B)
    for kw in (dict(cmd=None), dict(mean=None), dict(W=None)):
        rc = L.lib().cilrs_net_novelty(pl.handle, C.byref(pl.bufs),
                                       L.ptr(kw.get("cmd", cmd_d)), L.ptr(kw.get("mean", mean_d)),
                                       L.ptr(kw.get("W", W_d)), L.ptr(out.d2), L.ptr(out.scratch), out.n,
                                       _st())
        assert rc != 0 and "NULL" in _err(), (kw, _err())
        out.untouched()
    table, check = G.guarded(N.table_doubles(F, NC), dtype=torch.float64, name="table")
    assert _net_moments(pl, None, piv_d, table) != 0 and "NULL" in _err()
    assert _net_moments(pl, cmd_d, None, table) != 0 and "NULL" in _err()
    check()
    assert bool(torch.isnan(table).all())
    # ... and the valid calls on the eval forward go through
    L.check(_net_novelty(pl, cmd_d, mean_d, W_d, out))
    out.check()
    G.all_finite(out.d2, "d2")


# ---- end to end --------------------------------------------------------------------------------------
def _fit_batches():
    """five batches of 3 and five of 5 frames at 40x120: N = 40"""
    return [O.synthetic_batch(B, seed=200 + 10 * B + i, h=40, w=120) for B in (3, 5) for i in range(5)]


def _fitted_density():
    if "density" not in _CACHE:
        from cilrs_mi355.novelty import FeatureDensity
        m, _orc = TM._pair()
        fd = FeatureDensity(m)
        feats = []
        for img, spd, cmd, _t, _u8 in _fit_batches():
            fd.update(img.cuda(), spd.cuda(), cmd.cuda())
            feats.append(_plan_features32(m.engine().last_plan, False))
        fd.finalize()
        _CACHE["density"] = (fd, feats)
    return _CACHE["density"]


def test_end_to_end_fit_and_predict_novelty(tmp_path):
    from cilrs_mi355.novelty import FeatureDensity
    from cilrs_mi355.predict import Predictor, SPEED_NORM_FACTOR
    m, _orc = TM._pair()
    fd, fit_feats = _fitted_density()
    batches = _fit_batches()
    F, NC = 512, 4
    assert fd.finalized and fd.count == 40 and fd.F == F and fd.NC == NC
    # the device's table against the definition on the features the forwards left
    v_all = np.concatenate(fit_feats)
    cmd_all = np.concatenate([b[2].numpy() for b in batches])
    piv = fd.pivot.cpu().numpy()
    assert np.abs(piv - fit_feats[0].mean(axis=0, dtype=np.float64)).max() <= 1e-6
    n, s, Gd = N.split(fd.table.cpu().numpy(), F, NC)
    nr, sr, Gr = N.split(N.moments(v_all, cmd_all, piv, NC), F, NC)
    bG, _bx = N.moments_bound(v_all, piv)
    assert np.array_equal(n, nr) and (np.abs(np.tril(Gd) - np.tril(Gr)) <= bG).all()
    fin = N.finalize(fd.table.cpu().numpy(), piv, F, NC, fd.shrinkage)
    assert np.array_equal(fin["present"], fd.present)
    relw = np.abs(fd.W.cpu().numpy() - fin["W32"]).max() / np.abs(fin["W32"]).max()
    print(f"end to end: W against the definition's {relw:.3g}")
    assert relw <= 1e-6
    # score the same frames through Predictor.predict_novelty
    mean32, W32 = fd.mean.cpu().numpy(), fd.W.cpu().numpy()
    preds = {B: Predictor(m, batch=B, height=40, width=120, persistent=False) for B in (3, 5)}
    d2_all, bound_all, drift = [], [], 0.0
    for (img, spd, cmd, _t, u8), vfit in zip(batches, fit_feats):
        pred = preds[len(cmd)]
        kmh = (spd.double() * SPEED_NORM_FACTOR).numpy()
        controls, pspeed, d2 = pred.predict_novelty(u8, kmh, cmd.numpy(), fd)
        assert controls.shape == (len(cmd), 3) and pspeed.shape == d2.shape == (len(cmd),)
        assert controls.dtype == pspeed.dtype == d2.dtype == np.float32
        v = _plan_features32(pred.eng.last_plan, False)
        drift = max(drift, float(np.abs(v - vfit).max()))
        ref, bound = N.score(v, cmd.numpy(), mean32, W32)
        assert (np.abs(d2.astype(np.float64) - ref) <= bound).all()
        point = pred.predict_batch(u8, kmh, cmd.numpy())
        assert np.array_equal(controls, point[:, :3]) and np.array_equal(pspeed, point[:, 3])
        d2_all.append(d2.astype(np.float64))
        bound_all.append(bound)
    d2_all, bound_all = np.concatenate(d2_all), np.concatenate(bound_all)
    # trace identity: sum_n d2_n = tr(Sigma_l^-1 S_w), so the mean over the fit set is
    # tr(Sigma_l^-1 Sigma) (N - K') / N -- from the device's own table in float64
    Nn, Kp = fin["N"], fin["Kp"]
    want = np.trace(np.linalg.solve(fin["sigma_l"], fin["sigma"])) * (Nn - Kp) / Nn
    print(f"end to end: mean d2 {d2_all.mean():.6f}, trace identity {want:.6f}, bound "
          f"{bound_all.mean():.3g}, features of the u8 path against the fit's {drift:.3g}")
    assert abs(d2_all.mean() - want) <= bound_all.mean()
    # calibration: percentile is monotone and has a meaning
    fd.calibrate([(b[0].cuda(), b[1].cuda(), b[2].cuda()) for b in batches[:2] + batches[5:7]])
    assert fd.log_count == 16
    s = fd.calibration_scores()
    grid = np.linspace(0.0, 2.0 * float(s[-1]), 50, dtype=np.float32)
    pc = fd.percentile(grid)
    assert np.all(np.diff(pc) >= 0) and pc[0] == 0.0 and pc[-1] == 100.0
    assert fd.quantile(0.0) == s[0] and fd.quantile(1.0) == s[-1]
    assert s[0] <= fd.quantile(0.5) <= s[-1]
    # save / load reproduces d2 bit for bit
    path = tmp_path / "density.pth"
    fd.save(path)
    fd2 = FeatureDensity(m)
    fd2.load(path)
    assert torch.equal(fd2.W, fd.W) and torch.equal(fd2.mean, fd.mean)
    assert np.array_equal(fd2.calibration_scores(), s)
    img, spd, cmd, _t, u8 = batches[7]
    kmh = (spd.double() * SPEED_NORM_FACTOR).numpy()
    a = preds[5].predict_novelty(u8, kmh, cmd.numpy(), fd)[2]
    b = preds[5].predict_novelty(u8, kmh, cmd.numpy(), fd2)[2]
    assert np.array_equal(a, b)


def test_predictor_forms_and_refusals():
    from cilrs_mi355.novelty import FeatureDensity
    from cilrs_mi355.predict import Predictor
    m, _orc = TM._pair()
    fd, _feats = _fitted_density()
    mean32, W32 = fd.mean.cpu().numpy(), fd.W.cpu().numpy()
    pred = Predictor(m)                                      # the persistent single-frame predictor
    assert pred.persistent
    u8 = O.synthetic_batch(1, seed=60)[4]                    # 88 x 200 x 3
    controls, pspeed, d2 = pred.predict_novelty(u8, [30.0], [2], fd)
    pl = pred.eng.plan(1, 88, 200)
    ref, bound = N.score(_plan_features32(pl, True), [2], mean32, W32)
    print(f"persistent 88x200: d2 {float(d2[0]):.6g} (definition {ref[0]:.6g}, bound {bound[0]:.3g})")
    assert abs(float(d2[0]) - ref[0]) <= bound[0]
    point = pred.predict_batch(u8, [30.0], [2])
    assert np.array_equal(controls, point[:, :3]) and np.array_equal(pspeed, point[:, 3])
    # the camera-frame form: an 88x200 frame, then a frame that goes through predict_camera's path
    tick, one = pred.predict_controls_novelty(u8[0], 30.0, 2, fd)
    assert isinstance(one, float) and one == float(d2[0])
    assert tick == pred.predict_controls(u8[0], 30.0, 2)
    cam = O.synthetic_batch(1, seed=43, h=50, w=300)[4][0]
    tick_c, d2_c = pred.predict_controls_novelty(cam, 33.0, 3, fd)
    ref_c, bound_c = N.score(_plan_features32(pl, True), [3], mean32, W32)
    assert abs(d2_c - ref_c[0]) <= bound_c[0] and len(tick_c) == 4
    # a degraded tick is served through the per-layer launches, whose features sit in `combined`
    pred._inject_timeout = 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        controls_d, _ps, d2_d = pred.predict_novelty(u8, [30.0], [2], fd)
        assert pred.barrier_timeouts == 1 and pred.degraded_ticks_left > 0
        ref_d, bound_d = N.score(_plan_features32(pl, False), [2], mean32, W32)
        assert abs(float(d2_d[0]) - ref_d[0]) <= bound_d[0]
        assert np.array_equal(controls_d, pred.predict_batch(u8, [30.0], [2])[:, :3])
    # the per-layer trunk rounds differently from the persistent launch: close, not equal
    assert abs(float(d2_d[0]) - float(d2[0])) <= 1e-2 * float(d2[0])
    # refusals, before anything is launched
    with pytest.raises(RuntimeError, match="fp32 predictors only"):
        Predictor(m, batch=2, height=40, width=120, half=True).predict_novelty(
            O.synthetic_batch(2, seed=1, h=40, w=120)[4], [10.0, 20.0], [0, 1], fd)
    with pytest.raises(RuntimeError, match="finalize"):
        pred.predict_novelty(u8, [30.0], [2], FeatureDensity(m))
    m50, _o = TM._models50()
    with pytest.raises(RuntimeError, match="features"):
        Predictor(m50, batch=1, height=40, width=120).predict_novelty(
            O.synthetic_batch(1, seed=1, h=40, w=120)[4], [10.0], [0], fd)
    with pytest.raises(RuntimeError, match="out of range"):
        pred.predict_novelty(u8, [30.0], [4], fd)
    gap = FeatureDensity(m)
    gap.load_state_dict(fd.state_dict())
    gap.present = np.array([True, True, False, True])
    with pytest.raises(RuntimeError, match="never occurred"):
        pred.predict_novelty(u8, [30.0], [2], gap)
    with pytest.raises(RuntimeError, match="single-frame"):
        Predictor(m, batch=2, height=40, width=120).predict_controls_novelty(u8[0], 30.0, 2, fd)
