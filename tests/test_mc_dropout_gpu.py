"""Monte-Carlo dropout through the heads on the device (csrc/mc_heads.hip: cilrs_heads_mc,
cilrs_net_heads_mc, Predictor.predict_uncertain) against the float64 definition of
tests/_mc_dropout.py.

Gates.  Every sample within 2e-5 * max(1, max|ref|) of the float64 definition (the project's gate
for the heads against float64; the fp32 CPU realisation of the same definition
sits 1.6e-7 .. 1.4e-6 away, tests/test_mc_dropout_host.py prints it).  mean / std within
1e-6 * max(1, |ref|) of the float64 statistics of the kernel's OWN stored samples (one fp32 rounding
of a double result is 6e-8 relative).  Outputs are NaN-pre-filled inside guard bands
(tests/_guards.py) and the scratch is exactly sized.

cilrs_dropout serves sites 0..9 only (it is an existing entry point and stays as it is), so the masks
are read back through it for those sites; the sites of a sixth command (11 .. 13) are held to the
documented hash on the CPU (tests/test_mc_dropout_host.py) and through the samples themselves.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _guards as G
import _mc_dropout as D
import cilrs_oracle as O

pytestmark = pytest.mark.gpu

SEED = 0x0DDC0FFEE123
_CACHE = {}


def _lib():
    from cilrs_mi355 import _lib as L
    return L


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err():
    msg = _lib().lib().cilrs_last_error()
    return msg.decode() if msg else ""


def _heads(nc, feat):
    key = ("heads", nc, feat)
    if key not in _CACHE:
        _CACHE[key] = D.build_heads(nc, feat, seed=nc)
    return _CACHE[key]


def _arena(code, hm):
    """Device parameter arena of architecture `code` holding hm's head weights (the trunk's stay
    zero: the op-level entry does not read them)."""
    key = ("arena", code)
    if key in _CACHE:
        return _CACHE[key]
    L = _lib()
    lib = L.lib()
    arena = torch.zeros(lib.cilrs_variant_param_arena_floats(code), dtype=torch.float32)
    sd, seen = hm.state_dict(), set()
    name = C.create_string_buffer(160)
    off, numel, ndim, shape = L.sz(), L.sz(), L.i32(), (L.i32 * 4)()
    for i in range(lib.cilrs_variant_num_params(code)):
        L.check(lib.cilrs_variant_param_info(code, i, name, 160, C.byref(off), C.byref(numel),
                                             C.byref(ndim), shape))
        nm = name.value.decode()
        if nm in sd:
            assert numel.value == sd[nm].numel(), nm
            arena[off.value:off.value + numel.value] = sd[nm].reshape(-1)
            seen.add(nm)
    assert seen == set(sd), set(sd) - seen
    _CACHE[key] = arena.cuda()
    return _CACHE[key]


def _pooled_dev(v, ld):
    """[B][ld] on the device, features first, the pad columns NaN (they must not be read)"""
    t = torch.full((v.size(0), ld), float("nan"), dtype=torch.float32)
    t[:, :v.size(1)] = v
    return t.cuda()


class _Out:
    """guarded, NaN-filled mean / std / samples_out and an exactly sized, NaN-filled scratch"""

    def __init__(self, code, B, S, want_samples=True, scratch_short=0):
        L = _lib()
        self.B, self.S = B, S
        self.n = L.lib().cilrs_heads_mc_scratch_floats(code, B, S)
        self.mean, c1 = G.guarded(B * 4, name="mean")
        self.std, c2 = G.guarded(B * 4, name="std")
        self.smp, c3 = G.guarded(B * S * 4 if want_samples else 0, name="samples_out")
        self.scratch, c4 = G.guarded(max(self.n - scratch_short, 1), name="scratch")
        self.want = want_samples
        self.checks = (c1, c2, c3, c4)

    def ptrs(self):
        L = _lib()
        return (L.ptr(self.mean), L.ptr(self.std), L.ptr(self.smp) if self.want else None,
                L.ptr(self.scratch))

    def check(self):
        for c in self.checks:
            c()

    def untouched(self):
        self.check()
        for t in (self.mean, self.std, self.smp, self.scratch):
            assert bool(torch.isnan(t).all()), "a refused call wrote to its outputs"

    def results(self):
        self.check()
        G.all_finite(self.mean, "mean")
        G.all_finite(self.std, "std")
        if self.want:
            G.all_finite(self.smp, "samples_out")
        return (self.mean.cpu().view(self.B, 4), self.std.cpu().view(self.B, 4),
                self.smp.cpu().view(self.B, self.S, 4) if self.want else None)


def _run_op(code, arena, pooled_d, ld, spd_d, cmd_d, S, p, seed, want_samples=True):
    L = _lib()
    B = spd_d.numel()
    out = _Out(code, B, S, want_samples)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ins = G.Inputs(pooled=pooled_d, speed=spd_d, command=cmd_d)
    mean, std, smp, scratch = out.ptrs()
    L.check(L.lib().cilrs_heads_mc(code, L.ptr(arena), L.ptr(pooled_d), ld, L.ptr(spd_d),
                                   L.ptr(cmd_d), B, S, p, seed, mean, std, smp, scratch, out.n,
                                   L.ptr(status), _st()))
    ins.check()
    return out.results() + (int(status.item()),)


def _check_samples(got, ref, what):
    bound = D.TOL * max(1.0, float(ref.abs().max()))
    err = float((got.double() - ref).abs().max())
    print(f"MC {what}: samples max err {err:.3g} (bound {bound:.3g}, max|ref| {float(ref.abs().max()):.3g}, "
          f"std over samples {float(ref.std(dim=1).min()) if ref.size(1) > 1 else 0.0:.3g}+)")
    assert err <= bound, (what, err, bound)


def _check_stats(mean, std, smp, what):
    m64, s64 = D.stats64(smp)
    em = float(((mean.double() - m64).abs() / m64.abs().clamp(min=1.0)).max())
    es = float(((std.double() - s64).abs() / s64.abs().clamp(min=1.0)).max())
    print(f"MC {what}: mean err {em:.3g}, std err {es:.3g} (bound {D.TOL_STATS:.3g})")
    assert em <= D.TOL_STATS and es <= D.TOL_STATS, (what, em, es)
    if smp.size(1) == 1:
        assert torch.equal(std, torch.zeros_like(std))
        assert torch.equal(mean, smp[:, 0])


def _check_masks_on_device(B, S, p, seed, site_cols):
    """the CPU masks the reference used == what cilrs_dropout returns on ones [B*S][cols]"""
    L = _lib()
    rows = B * S
    for site, cols in site_cols:
        assert site <= 9
        ones = torch.ones(rows, cols, dtype=torch.float32, device="cuda")
        L.check(L.lib().cilrs_dropout(L.ptr(ones), rows, cols, cols, p, seed, site, _st()))
        torch.cuda.synchronize()
        got = ones.cpu().numpy() != 0.0
        assert np.array_equal(got, D.keep(seed, site, rows, cols, p)), f"site {site}"


# ---- op level against float64 ----------------------------------------------------------------------
GRID = [(B, S, p) for B in (1, 3) for S in (1, 5, 33, 70) for p in (0.5, 0.25)]
assert {(i + j) % 4 for i, (B, _s, _p) in enumerate(GRID) for j in range(B)} == {0, 1, 2, 3}


@pytest.mark.parametrize("B,S,p", GRID)
def test_op_level_against_float64(B, S, p):
    i = GRID.index((B, S, p))
    hm = _heads(4, 512)
    arena = _arena(0, hm)
    v, spd = D.synthetic_features(B, 512, seed=5 + i)
    cmd = torch.tensor([(i + j) % 4 for j in range(B)], dtype=torch.int64)
    ld = 512 if i % 2 else 640
    pooled_d, spd_d, cmd_d = _pooled_dev(v, ld), spd.cuda(), cmd.cuda()
    seed = SEED + i
    mean, std, smp, status = _run_op(0, arena, pooled_d, ld, spd_d, cmd_d, S, p, seed)
    assert status == 0
    what = f"op B={B} S={S} p={p}"
    ref = D.mc_samples(hm, v, spd, cmd, S, p, seed)
    _check_samples(smp, ref, what)
    _check_stats(mean, std, smp, what)
    mean2, std2, _none, _ = _run_op(0, arena, pooled_d, ld, spd_d, cmd_d, S, p, seed,
                                    want_samples=False)
    assert torch.equal(mean2, mean) and torch.equal(std2, std)
    sites = {(0, 128), (9, 256)}
    for k in set(cmd.tolist()):
        sites |= {(1 + 2 * k, 256), (2 + 2 * k, 256)}
    _check_masks_on_device(B, S, p, seed, sorted(sites))


ARCH_CASES = {
    "nc4_all_commands": (4 << 8, 4, 512, [0, 1, 2, 3]),
    "nc2": (2 << 8, 2, 512, [1, 0, 1]),
    "nc6": (6 << 8, 6, 512, [5, 2, 4]),
    "resnet50": (1, 4, 2048, [3, 1]),
}


@pytest.mark.parametrize("case", list(ARCH_CASES))
def test_op_level_architecture_codes(case):
    code, nc, feat, cmds = ARCH_CASES[case]
    B, S, p = len(cmds), 5, 0.5
    hm = _heads(nc, feat)
    arena = _arena(code, hm)
    v, spd = D.synthetic_features(B, feat, seed=17)
    cmd = torch.tensor(cmds, dtype=torch.int64)
    ld = feat + 128
    mean, std, smp, status = _run_op(code, arena, _pooled_dev(v, ld), ld, spd.cuda(), cmd.cuda(), S, p,
                                     SEED)
    assert status == 0
    ref = D.mc_samples(hm, v, spd, cmd, S, p, SEED)
    _check_samples(smp, ref, f"op {case}")
    _check_stats(mean, std, smp, f"op {case}")
    st = D.sites(nc)
    sites = {(0, 128)} | {(s, 256) for k in set(cmds) for s in st[f"control_branches.{k}"]}
    sites |= {(st["speed_predictor"][0], 256)}
    _check_masks_on_device(B, S, p, SEED, sorted(s for s in sites if s[0] <= 9))


def test_bad_command_uses_branch_zero_and_sets_the_status_word():
    hm = _heads(4, 512)
    arena = _arena(0, hm)
    v, spd = D.synthetic_features(2, 512, seed=3)
    cmd = torch.tensor([7, -1], dtype=torch.int64)
    mean, std, smp, status = _run_op(0, arena, _pooled_dev(v, 512), 512, spd.cuda(), cmd.cuda(), 5, 0.5,
                                     SEED)
    assert status == 1
    ref = D.mc_samples(hm, v, spd, torch.zeros(2, dtype=torch.int64), 5, 0.5, SEED)
    _check_samples(smp, ref, "op bad command")


# ---- grouping independence, determinism, p = 0 ---------------------------------------------------
def test_grouping_independence_and_determinism():
    hm = _heads(4, 512)
    arena = _arena(0, hm)
    v, spd = D.synthetic_features(1, 512, seed=8)
    cmd = torch.tensor([2], dtype=torch.int64)
    args = (0, arena, _pooled_dev(v, 512), 512, spd.cuda(), cmd.cuda())
    _m70, _s70, smp70, _ = _run_op(*args, 70, 0.5, SEED)
    m33, s33, smp33, _ = _run_op(*args, 33, 0.5, SEED)
    assert torch.equal(smp70[:, :33], smp33)          # a row does not know how many rows there are
    m33b, s33b, smp33b, _ = _run_op(*args, 33, 0.5, SEED)
    assert torch.equal(smp33b, smp33) and torch.equal(m33b, m33) and torch.equal(s33b, s33)
    _m, _s, other, _ = _run_op(*args, 33, 0.5, SEED + 1)
    assert not torch.equal(other, smp33)
    assert float((other - smp33).abs().max()) > 0.05
    # one tile's worth of samples takes its statistics inside the sample launch, more take the
    # statistics launch: both are the same two passes
    _m32, _s32, smp32, _ = _run_op(*args, 32, 0.5, SEED)
    assert torch.equal(smp32, smp33[:, :32])


@pytest.mark.parametrize("B,S", [(1, 5), (3, 33), (2, 70)])
def test_p_zero_is_the_eval_output_and_std_is_zero(B, S):
    hm = _heads(4, 512)
    arena = _arena(0, hm)
    v, spd = D.synthetic_features(B, 512, seed=11)
    cmd = torch.tensor([(3 - j) % 4 for j in range(B)], dtype=torch.int64)
    mean, std, smp, _ = _run_op(0, arena, _pooled_dev(v, 640), 640, spd.cuda(), cmd.cuda(), S, 0.0, SEED)
    for s in range(S):
        assert torch.equal(smp[:, s], smp[:, 0])
    assert torch.equal(std, torch.zeros_like(std))
    assert torch.equal(mean, smp[:, 0])
    ref = D.eval_outputs(hm, v, spd, cmd)
    _check_samples(smp[:, :1], ref.unsqueeze(1), f"op p=0 B={B} S={S}")


# ---- refusals -----------------------------------------------------------------------------------------
def _refusal_args():
    hm = _heads(4, 512)
    arena = _arena(0, hm)
    v, spd = D.synthetic_features(2, 512, seed=3)
    return dict(code=0, arena=arena, pooled=_pooled_dev(v, 512), ld=512, speed=spd.cuda(),
                command=torch.tensor([1, 2], dtype=torch.int64).cuda(), B=2, S=5, p=0.5)


REFUSALS = {
    "null params": (dict(arena=None), "NULL"),
    "null pooled": (dict(pooled=None), "NULL"),
    "null speed": (dict(speed=None), "NULL"),
    "null command": (dict(command=None), "NULL"),
    "null mean": (dict(null_out="mean"), "NULL"),
    "null std": (dict(null_out="std"), "NULL"),
    "samples 0": (dict(S=0), "samples"),
    "samples 4097": (dict(S=4097), "samples"),
    "rows above 65536": (dict(B=17, S=4096), "batch * samples"),
    "p 1": (dict(p=1.0), "probability"),
    "p negative": (dict(p=-0.125), "probability"),
    "p nan": (dict(p=float("nan")), "probability"),
    "p inf": (dict(p=float("inf")), "probability"),
    "scratch one float short": (dict(short=1), "scratch"),
    "null scratch": (dict(null_out="scratch"), "scratch"),
    "unknown trunk": (dict(code=2), "architecture code"),
    "nine commands": (dict(code=9 << 8), "architecture code"),
    "negative code": (dict(code=-1), "architecture code"),
    "pooled_ld below the features": (dict(ld=511), "pooled_ld"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_op_level_refusals_launch_nothing(case):
    change, text = REFUSALS[case]
    a = _refusal_args()
    null_out, short = change.pop("null_out", None), change.pop("short", 0)
    a.update(change)
    L = _lib()
    # the buffers are those of the valid call: a refused call must not touch them whatever it was told
    out = _Out(0, 2, 5, True, scratch_short=short)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    mean, std, smp, scratch = out.ptrs()
    n = out.n - short
    if null_out == "mean":
        mean = None
    elif null_out == "std":
        std = None
    elif null_out == "scratch":
        scratch = None
    rc = L.lib().cilrs_heads_mc(a["code"], L.ptr(a["arena"]), L.ptr(a["pooled"]), a["ld"],
                                L.ptr(a["speed"]), L.ptr(a["command"]), a["B"], a["S"], a["p"], SEED,
                                mean, std, smp, scratch, n, L.ptr(status), _st())
    msg = _err()
    assert rc != 0, case
    assert text in msg, (case, msg)
    out.untouched()
    assert int(status.item()) == 0


def test_scratch_size_query():
    lib = _lib().lib()
    assert lib.cilrs_heads_mc_scratch_floats(0, 3, 70) > 3 * 70 * 4
    assert lib.cilrs_heads_mc_scratch_floats(2, 3, 70) == 0
    assert lib.cilrs_heads_mc_scratch_floats(0, 0, 70) == 0
    assert lib.cilrs_heads_mc_scratch_floats(0, 3, 0) == 0


# ---- plan level --------------------------------------------------------------------------------------
def _pair():
    import test_eval32_layers_gpu as T32
    return T32._pair()


def _plan_view(pl):
    import test_eval32_layers_gpu as T32
    return T32._PlanView(pl)


def _stored_features(pl, source, last_conv=35):
    """float64 pooled features of the forward that just ran on the plan: the average of the last
    feature map it stored ("map"), or the fp32 `combined` it pooled itself ("combined")."""
    L = _lib()
    if source == "map":
        return _plan_view(pl).fetch(last_conv).double().mean(dim=2)
    co, ld, feat = L.sz(), L.i32(), L.i32()
    L.check(L.lib().cilrs_net_infer16_io_info(pl.handle, None, None, C.byref(co), C.byref(ld),
                                              C.byref(feat)))
    comb = pl.workspace[co.value:co.value + 4 * pl.batch * ld.value].view(torch.float32)
    return comb.view(pl.batch, ld.value)[:, :feat.value].cpu().double()


def _run_plan(pl, spd_d, cmd_d, S, p, seed, want_samples=True, expect_rc0=True):
    L = _lib()
    out = _Out(0, pl.batch, S, want_samples)
    mean, std, smp, scratch = out.ptrs()
    rc = L.lib().cilrs_net_heads_mc(pl.handle, C.byref(pl.bufs), L.ptr(spd_d), L.ptr(cmd_d), S, p,
                                    seed, mean, std, smp, scratch, out.n, _st())
    if not expect_rc0:
        return rc, out
    L.check(rc)
    return out.results()


def _fwd_per_layer(eng, u8, spd, cmd):
    return eng.run_forward_u8(u8, spd, cmd, graph=False, half=False, persistent=False)


def _fwd_persistent(eng, u8, spd, cmd):
    return eng.run_forward_u8(u8, spd, cmd, persistent=True)


def _fwd_f16(eng, u8, spd, cmd):
    return eng.run_forward_u8(u8, spd, cmd, half=True)


def _fwd_bf16(eng, u8, spd, cmd):
    return eng.run_forward_u8(u8, spd, cmd, half="bf16")


def _fwd_frozen(eng, u8, spd, cmd):
    return eng.run_forward_frozen_u8(u8, spd, cmd)[:2]


REALISATIONS = {
    "per_layer": (3, 40, 120, _fwd_per_layer, "map"),
    "persistent": (1, 30, 70, _fwd_persistent, "map"),
    "f16": (2, 40, 120, _fwd_f16, "combined"),
    "bf16": (2, 40, 120, _fwd_bf16, "combined"),
    "frozen": (3, 40, 120, _fwd_frozen, "map"),
}


@pytest.mark.parametrize("name", list(REALISATIONS))
def test_plan_level_after_each_eval_realisation(name):
    B, H, W, fwd, source = REALISATIONS[name]
    m, orc = _pair()
    eng = m.engine()
    _img, spd, cmd, _t, u8 = O.synthetic_batch(B, seed=77, h=H, w=W)
    u8_d, spd_d, cmd_d = torch.from_numpy(u8).cuda(), spd.cuda(), cmd.cuda()
    S, p = 33, 0.5
    ctrl, ps = fwd(eng, u8_d, spd_d, cmd_d)
    torch.cuda.synchronize()
    pl = eng.last_plan
    eng.check_status()
    before = (ctrl.clone(), ps.clone())
    pooled = _stored_features(pl, source)
    mean, std, smp = _run_plan(pl, spd_d, cmd_d, S, p, SEED)
    what = f"plan {name} ({B},{H},{W})"
    ref = D.mc_samples(orc, pooled, spd, cmd, S, p, SEED)
    _check_samples(smp, ref, what)
    _check_stats(mean, std, smp, what)
    # the forward's own outputs: untouched by the MC launches, and the same from the next forward
    assert torch.equal(ctrl, before[0]) and torch.equal(ps, before[1])
    ctrl2, ps2 = fwd(eng, u8_d, spd_d, cmd_d)
    torch.cuda.synchronize()
    assert torch.equal(ctrl2, before[0]) and torch.equal(ps2, before[1])
    # p = 0: every sample is the eval output
    mean0, std0, smp0 = _run_plan(pl, spd_d, cmd_d, 3, 0.0, SEED)
    assert torch.equal(smp0[:, 1], smp0[:, 0]) and torch.equal(smp0[:, 2], smp0[:, 0])
    assert torch.equal(std0, torch.zeros_like(std0)) and torch.equal(mean0, smp0[:, 0])
    own = torch.cat([before[0].cpu(), before[1].cpu().view(-1, 1)], dim=1)
    err0 = float((mean0 - own).abs().max())
    print(f"MC {what}: p = 0 mean vs the forward's outputs {err0:.3g}")
    assert err0 <= D.TOL * max(1.0, float(own.abs().max()))
    # a command of 7: status word 0, branch 0
    assert pl.status.tolist()[0] == 0
    bad = cmd.clone()
    bad[0] = 7
    _m, _s, smp_bad = _run_plan(pl, spd_d, bad.cuda(), 5, p, SEED)
    assert pl.status.tolist()[0] == 1
    pl.status.zero_()
    torch.cuda.synchronize()
    ref_bad = D.mc_samples(orc, pooled, spd, bad, 5, p, SEED)        # (the helper maps 7 to branch 0)
    _check_samples(smp_bad, ref_bad, what + " command 7")
    zero = cmd.clone()
    zero[0] = 0
    assert float((ref_bad - D.mc_samples(orc, pooled, spd, zero, 5, p, SEED)).abs().max()) < 1e-12


def _train_model():
    if "train_model" not in _CACHE:
        from cilrs_mi355 import CILRS
        torch.manual_seed(0)
        _CACHE["train_model"] = CILRS(4, 0.5).cuda()
    return _CACHE["train_model"]


def test_plan_level_refusals():
    m = _train_model()
    eng = m.engine()
    B, H, W = 3, 40, 120
    img, spd, cmd, _t, _u8 = O.synthetic_batch(B, seed=5, h=H, w=W)
    spd_d, cmd_d = spd.cuda(), cmd.cuda()
    pl = eng.plan(B, H, W, lane=3)                     # a plan no forward has run on
    rc, out = _run_plan(pl, spd_d, cmd_d, 5, 0.5, SEED, expect_rc0=False)
    assert rc != 0 and "no forward" in _err(), _err()
    out.untouched()
    _c, _s, pl = eng.run_forward(img.cuda(), spd_d, cmd_d, True, 0.5, 1)
    torch.cuda.synchronize()
    rc, out = _run_plan(pl, spd_d, cmd_d, 5, 0.5, SEED, expect_rc0=False)
    assert rc != 0 and "train mode" in _err(), _err()
    out.untouched()
    eng.run_forward(img.cuda(), spd_d, cmd_d, False, 0.0, 0)
    torch.cuda.synchronize()
    for kw, text in ((dict(S=0), "samples"), (dict(S=4097), "samples"), (dict(p=1.0), "probability"),
                     (dict(p=float("nan")), "probability")):
        L = _lib()
        out = _Out(0, B, 5)
        mean, std, smp, scratch = out.ptrs()
        rc = L.lib().cilrs_net_heads_mc(pl.handle, C.byref(pl.bufs), L.ptr(spd_d), L.ptr(cmd_d),
                                        kw.get("S", 5), kw.get("p", 0.5), SEED, mean, std, smp, scratch,
                                        out.n, _st())
        assert rc != 0 and text in _err(), (kw, _err())
        out.untouched()
    L = _lib()
    out = _Out(0, B, 5, scratch_short=1)
    mean, std, smp, scratch = out.ptrs()
    rc = L.lib().cilrs_net_heads_mc(pl.handle, C.byref(pl.bufs), L.ptr(spd_d), L.ptr(cmd_d), 5, 0.5,
                                    SEED, mean, std, smp, scratch, out.n - 1, _st())
    assert rc != 0 and "scratch" in _err()
    out.untouched()
    rc = L.lib().cilrs_net_heads_mc(pl.handle, C.byref(pl.bufs), None, L.ptr(cmd_d), 5, 0.5, SEED,
                                    mean, std, smp, scratch, out.n, _st())
    assert rc != 0 and "NULL" in _err()
    out.untouched()
    # ... and the valid call on the eval forward goes through
    mean, std, smp = _run_plan(pl, spd_d, cmd_d, 5, 0.5, SEED)
    assert float(std.min()) > 0.0


# ---- Predictor ---------------------------------------------------------------------------------------
def _models50():
    if "pair50" not in _CACHE:
        from test_infer16_gpu import _models
        _CACHE["pair50"] = _models("resnet50")
    return _CACHE["pair50"]


PREDICTORS = {
    # name: (network, batch, H, W, Predictor keywords, where the definition takes its features)
    "persistent": ("resnet34", 1, 88, 200, dict(), "map"),
    "per_layer": ("resnet34", 3, 40, 120, dict(persistent=False), "map"),
    "use_graph": ("resnet34", 1, 40, 120, dict(use_graph=True, persistent=False), "map"),
    "half": ("resnet34", 2, 40, 120, dict(half=True), "combined"),
    "resnet50": ("resnet50", 1, 40, 120, dict(), "combined"),
}


def _std_bound(gate, S):
    # |std(x + d) - std(x)| <= sqrt(sum d_s^2 / (S - 1)) <= max|d| * sqrt(S / (S - 1)): the centred
    # norm is a norm.  Plus the fp32 rounding of the result.
    return gate * math.sqrt(S / (S - 1.0))


def _check_predictor_result(r, pred, orc, source, spd_kmh, cmds, S, p, seed, what):
    from cilrs_mi355.predict import SPEED_NORM_FACTOR
    eng = pred.eng
    pl = eng.plan(pred.batch, pred.frames_host.size(1), pred.frames_host.size(2))
    last_conv = 35
    pooled = _stored_features(pl, source, last_conv)
    spd = torch.from_numpy(np.minimum(np.asarray(spd_kmh, dtype=np.float64) / SPEED_NORM_FACTOR,
                                      1.0).astype(np.float32))
    cmd = torch.tensor(cmds, dtype=torch.int64)
    ref = D.mc_samples(orc, pooled, spd, cmd, S, p, seed)
    gate = D.TOL * max(1.0, float(ref.abs().max()))
    scale = torch.tensor([1.0, 1.0, 1.0, SPEED_NORM_FACTOR], dtype=torch.float64)
    ref_kmh = ref * scale
    m64, s64 = D.stats64(ref.float())
    em = float(((torch.from_numpy(r["mean"]).double() - m64 * scale).abs() / scale).max())
    es = float(((torch.from_numpy(r["std"]).double() - s64 * scale).abs() / scale).max())
    print(f"MC predictor {what}: mean err {em:.3g}, std err {es:.3g} (gate {gate:.3g})")
    assert em <= gate + D.TOL_STATS * float(m64.abs().max())
    assert es <= _std_bound(gate, S) + D.TOL_STATS * float(s64.abs().max())
    if "samples" in r:
        e = float(((torch.from_numpy(r["samples"]).double() - ref_kmh).abs() / scale).max())
        assert e <= gate, (what, e)
    for k in ("point", "mean", "std"):
        assert r[k].dtype == np.float32 and r[k].shape == (pred.batch, 4), k


@pytest.mark.parametrize("name", list(PREDICTORS))
def test_predictor_predict_uncertain(name):
    from cilrs_mi355.predict import Predictor
    net, B, H, W, kw, source = PREDICTORS[name]
    m, orc = _pair() if net == "resnet34" else _models50()
    pred = Predictor(m, batch=B, height=H, width=W, **kw)
    u8 = O.synthetic_batch(B, seed=31, h=H, w=W)[4]
    kmh = [12.0 + 40.0 * j for j in range(B)]               # (the last of three is clipped to 1.0)
    cmds = [(2 + j) % 4 for j in range(B)]
    S, p, seed = 33, 0.5, 5
    r = pred.predict_uncertain(u8, kmh, cmds, samples=S, p=p, seed=seed, return_samples=True)
    assert set(r) == {"point", "mean", "std", "samples"}
    assert r["samples"].shape == (B, S, 4) and r["samples"].dtype == np.float32
    _check_predictor_result(r, pred, orc, source, kmh, cmds, S, p, seed, name)
    assert np.array_equal(r["point"], pred.predict_batch(u8, kmh, cmds))
    # column 3 is km/h: the spread of the raw predicted speed times 90
    assert float(r["std"][:, 3].min()) > 1.0
    r2 = pred.predict_uncertain(u8, kmh, cmds, samples=S, p=p, seed=seed)
    assert set(r2) == {"point", "mean", "std"}
    assert np.array_equal(r2["mean"], r["mean"]) and np.array_equal(r2["std"], r["std"])
    assert np.array_equal(r2["point"], r["point"])
    r3 = pred.predict_uncertain(u8, kmh, cmds, samples=S, p=p, seed=seed + 1)
    assert not np.array_equal(r3["mean"], r["mean"])


def test_predictor_arguments_and_model_dropout():
    from cilrs_mi355.predict import Predictor
    m, _orc = _pair()
    pred = Predictor(m, batch=1, height=40, width=120, persistent=False)
    u8 = O.synthetic_batch(1, seed=31, h=40, w=120)[4]
    with pytest.raises(ValueError, match="pass"):
        pred.predict_uncertain(u8, [10.0], [1])               # the pair's model has dropout = 0.0
    for kw in (dict(samples=0), dict(samples=4097), dict(samples=2.5), dict(p=1.0), dict(p=-0.1),
               dict(p=float("nan")), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            pred.predict_uncertain(u8, [10.0], [1], **{"p": 0.5, **kw})
    m2 = _train_model().eval()
    pred2 = Predictor(m2, batch=1, height=40, width=120, persistent=False)
    a = pred2.predict_uncertain(u8, [10.0], [1], samples=5)                  # p = model.dropout = 0.5
    b = pred2.predict_uncertain(u8, [10.0], [1], samples=5, p=0.5)
    c = pred2.predict_uncertain(u8, [10.0], [1], samples=5, p=0.25)
    assert np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["std"], b["std"])
    assert not np.array_equal(a["std"], c["std"])


def test_predict_controls_uncertain():
    from cilrs_mi355.predict import Predictor
    m, orc = _pair()
    pred = Predictor(m)                                      # the persistent single-frame predictor
    frame = O.synthetic_batch(1, seed=41)[4][0]              # 88 x 200 x 3
    S, p, seed = 16, 0.5, 9
    mean, std = pred.predict_controls_uncertain(frame, 33.0, 1, samples=S, p=p, seed=seed)
    assert len(mean) == 4 and len(std) == 4 and all(isinstance(x, float) for x in mean + std)
    r = pred.predict_uncertain(frame[None], [33.0], [1], samples=S, p=p, seed=seed)
    assert mean == tuple(float(x) for x in r["mean"][0]) and std == tuple(float(x) for x in r["std"][0])
    point = pred.predict_controls(frame, 33.0, 1)
    assert np.allclose(point, r["point"][0], rtol=0, atol=1e-5)
    # a camera-sized frame goes through predict_camera's path first
    cam = O.synthetic_batch(1, seed=43, h=50, w=300)[4][0]
    mean_c, std_c = pred.predict_controls_uncertain(cam, 33.0, 3, samples=S, p=p, seed=seed)
    rc = dict(point=np.zeros((1, 4), np.float32), mean=np.array([mean_c], np.float32),
              std=np.array([std_c], np.float32))
    _check_predictor_result(rc, pred, orc, "map", [33.0], [3], S, p, seed, "camera 50x300")
    assert min(std_c) > 0.0 and std_c[3] > 1.0
    with pytest.raises(ValueError):
        pred.predict_controls_uncertain(frame, 33.0, 1, samples=0, p=p)
