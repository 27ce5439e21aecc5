"""AdamW and LAMB on the device: cilrs_optim_table_create / cilrs_optim_step inside guard bands
against torch.optim.AdamW and against the two CPU statements of tests/_optim.py (float64, and fp32
in the header's operation order), position independence bit for bit, the refusals; then the Trainer:
one-step consistency on every route, data parallel per bucket, EMA behind the step, warm-up +
cosine through fit and a resume.

Tolerances.  AdamW: 1e-6 element-wise, the gate the project applies to cilrs_adam_step.  LAMB: the
trust ratio within 1e-6 relative of float64 (u carries about six roundings of 2^-24 and the norms
average them down; measured on these inputs: the fp32 CPU statement within 1.2e-7 relative of
float64, the device within 1.1e-7); per tensor max|device - float64| <= 8 * max(the same error of the fp32 CPU
statement of that tensor, 2^-24 * max|value|) for p, m and v -- the 8 allows for FMA contraction, the
device's divide and square-root sequences and one rounding of p (_optim.gate).
"""
import ctypes as C
import itertools

import pytest
import torch

import _ema as E
import _optim as Q
import cilrs_oracle as O
from _guards import Inputs, guarded

pytestmark = pytest.mark.gpu

# One workgroup covers one chunk: cilrs_optim_chunk_floats() = 4096 floats of one segment, in four
# trips of 256 threads x 4 floats.  L_SEG = 4100 is the smallest tensor that needs a second workgroup,
# whose partial sums the finalise adds to the first one's.  4092 / 4096 / 4100 straddle that edge,
# 3 * 4096 + 8 has three full chunks and a two-quad tail.
CHUNK = 4096
L_SEG = CHUNK + 4
SIZES = [4, 4, 64] + [64] * 40 + [4092, 4096, 4100, 3 * 4096 + 8, 4, L_SEG]
NSEG = len(SIZES)
ENDS = list(itertools.accumulate(SIZES))
STARTS = [0] + ENDS[:-1]
N = ENDS[-1]
PAD = {0: 1, 1: 1, 47: 1}            # biases of 3 padded to 4: trailing floats that are zero and stay zero
P0_SEG = 44                          # p == 0 everywhere
G0_SEG = 5                           # g == 0 on every step, NO_DECAY: nu == 0
GROUP_SPLIT = 20                     # two groups: segments [0, 20) and [20, NSEG)
GROUP_LR = (2e-3, 1e-3)
GROUP_STEP0 = (1, 4)
HP = dict(b1=0.9, b2=0.999, eps=1e-6, wd=1e-2)
assert N < 2_000_000 and SIZES[P0_SEG] == 4096 and SIZES[G0_SEG] == 64


def _L():
    from cilrs_mi355 import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def group_of(seg):
    return 0 if seg < GROUP_SPLIT else 1


def make_flags(flagged):
    """flagged: every segment of <= 64 floats carries NO_DECAY | NO_ADAPT; G0_SEG always NO_DECAY alone"""
    f = [(Q.NO_DECAY | Q.NO_ADAPT) if (flagged and s <= 64) else 0 for s in SIZES]
    f[G0_SEG] = Q.NO_DECAY
    return f


def pad_mask(sizes=SIZES, pad=PAD):
    keep = torch.ones(sum(sizes), dtype=torch.bool)
    ends = list(itertools.accumulate(sizes))
    for s, k in pad.items():
        keep[ends[s] - k:ends[s]] = False
    return keep


def make_state(seed, zero_moments):
    gen = torch.Generator().manual_seed(seed)
    keep = pad_mask()
    p = 0.05 * torch.randn(N, generator=gen)
    p[STARTS[P0_SEG]:ENDS[P0_SEG]] = 0.0
    if zero_moments:
        m, v = torch.zeros(N), torch.zeros(N)
    else:
        m = 1e-2 * torch.randn(N, generator=gen)
        v = 1e-3 * torch.rand(N, generator=gen)
    return p * keep, m * keep, v * keep


def make_grad(t):
    """mixed magnitude 1e-6 .. 1 with exact zeros, fresh on every step"""
    gen = torch.Generator().manual_seed(100 + t)
    g = torch.randn(N, generator=gen) * 10.0 ** torch.randint(-6, 1, (N,), generator=gen).float()
    g[::97] = 0.0
    g *= 3.0 / t
    g[STARTS[G0_SEG]:ENDS[G0_SEG]] = 0.0
    return g * pad_mask()


def gbuf(cpu, name):
    v, check = guarded(cpu.numel(), dtype=cpu.dtype, fill=None, guard=4096, name=name)
    v.copy_(cpu)
    return v, check


class Table:
    """a segment table in exactly sized, guarded device memory, with exactly sized scratch"""

    def __init__(self, sizes, flags):
        L = _L()
        lib = L.lib()
        self.ends = list(itertools.accumulate(sizes))
        self.n, self.k = self.ends[-1], len(sizes)
        c_ends, c_flags = (C.c_size_t * self.k)(*self.ends), (C.c_int * self.k)(*flags)
        nbytes = lib.cilrs_optim_table_bytes(c_ends, self.k)
        assert nbytes > 0 and nbytes % 16 == 0
        self.mem, self.check_mem = guarded(nbytes, dtype=torch.uint8, fill=None, name="table")
        self.h = C.c_void_p()
        L.check(lib.cilrs_optim_table_create(c_ends, c_flags, self.k, self.n, L.ptr(self.mem), nbytes,
                                             stream(), C.byref(self.h)))
        assert self.h.value
        sbytes = lib.cilrs_optim_scratch_bytes(self.h)
        assert sbytes == (nbytes // 16 - self.k) * 16 + 4 * self.k
        self.scratch, self.check_scratch = guarded(sbytes, dtype=torch.uint8, fill=None, name="scratch")
        self.ratios, self.check_ratios = guarded(self.k, fill=float("nan"), name="ratio_out")
        self.const = Inputs(table=self.mem)

    def check(self):
        self.check_mem(), self.check_scratch(), self.check_ratios()
        self.const.check()

    def close(self):
        _L().lib().cilrs_optim_table_destroy(self.h)
        self.h = None


def dev_step(kind, tab, first, count, p, g, m, v, groups, clip=None, gscale=1.0, trust_clip=0.0,
             scratch="own", ratios="own", table="own"):
    """groups: [(end in floats from the arena start, lr, step)]; returns the status"""
    L = _L()
    k = len(groups)
    return L.lib().cilrs_optim_step(
        kind, tab.h if table == "own" else table, first, count, L.ptr(p), L.ptr(g), L.ptr(m),
        L.ptr(v), k, (C.c_size_t * k)(*[x[0] for x in groups]),
        (C.c_double * k)(*[x[1] for x in groups]), (C.c_int64 * k)(*[x[2] for x in groups]),
        HP["b1"], HP["b2"], HP["eps"], HP["wd"], trust_clip, L.ptr(clip), gscale,
        L.ptr(tab.scratch) if scratch == "own" else scratch,
        L.ptr(tab.ratios) if ratios == "own" else ratios, stream())


def groups_for(first, count, steps):
    """the two groups restricted to the run [first, first + count)"""
    last = first + count
    if first < GROUP_SPLIT < last:
        return [(ENDS[GROUP_SPLIT - 1], GROUP_LR[0], steps[0]), (ENDS[last - 1], GROUP_LR[1], steps[1])]
    gi = group_of(first)
    return [(ENDS[last - 1], GROUP_LR[gi], steps[gi])]


CASES = pytest.mark.parametrize("clip_on,gscale", [(False, 1.0), (True, 0.5)], ids=["noclip", "clip"])
FLAGGED = pytest.mark.parametrize("flagged", [False, True], ids=["plain", "exempt"])


def test_chunk_constant():
    assert _L().lib().cilrs_optim_chunk_floats() == CHUNK


# ---- 1. AdamW against torch.optim.AdamW -----------------------------------------------------------
@CASES
@FLAGGED
def test_adamw_matches_torch_adamw(flagged, clip_on, gscale):
    L = _L()
    flags = make_flags(flagged)
    tab = Table(SIZES, flags)
    p0, m0, v0 = make_state(1, zero_moments=True)
    ref = [p0[b:e].clone().requires_grad_(True) for b, e in zip(STARTS, ENDS)]
    pg = []
    for gi in (0, 1):
        for exempt in (False, True):
            ps = [ref[s] for s in range(NSEG)
                  if group_of(s) == gi and bool(flags[s] & Q.NO_DECAY) == exempt]
            if ps:
                pg.append(dict(params=ps, lr=GROUP_LR[gi], weight_decay=0.0 if exempt else HP["wd"]))
    opt = torch.optim.AdamW(pg, betas=(HP["b1"], HP["b2"]), eps=HP["eps"], foreach=False)
    for s in range(GROUP_SPLIT, NSEG):           # the second group has three steps behind it
        opt.state[ref[s]] = dict(step=torch.tensor(float(GROUP_STEP0[1] - 1)),
                                 exp_avg=torch.zeros_like(ref[s]), exp_avg_sq=torch.zeros_like(ref[s]))
    (p, cp), (m, cm), (v, cv) = gbuf(p0, "params"), gbuf(m0, "exp_avg"), gbuf(v0, "exp_avg_sq")
    clip = torch.tensor([2.0, 0.5], device="cuda") if clip_on else None
    gs = Q.gscale32(0.5 if clip_on else None, gscale)
    worst = 0.0
    for t in range(1, 6):
        g_cpu = make_grad(t)
        g = g_cpu.cuda()
        const = Inputs(grads=g, clip_out2=clip)
        steps = (GROUP_STEP0[0] + t - 1, GROUP_STEP0[1] + t - 1)
        L.check(dev_step(Q.ADAMW, tab, 0, NSEG, p, g, m, v, groups_for(0, NSEG, steps), clip, gscale,
                         scratch=None, ratios=None))
        cp(), cm(), cv(), tab.check(), const.check()
        for s in range(NSEG):
            ref[s].grad = g_cpu[STARTS[s]:ENDS[s]] * gs
        opt.step()
        for s in range(NSEG):
            assert int(opt.state[ref[s]]["step"]) == steps[group_of(s)]
        want = [torch.cat([r.detach() for r in ref]),
                torch.cat([opt.state[r]["exp_avg"] for r in ref]),
                torch.cat([opt.state[r]["exp_avg_sq"] for r in ref])]
        for name, got, w in zip(("p", "exp_avg", "exp_avg_sq"), (p, m, v), want):
            err = float((got.cpu() - w).abs().max())
            worst = max(worst, err)
            assert err <= 1e-6, f"step {t}: {name} differs from torch.optim.AdamW by {err:.3e}"
    print(f"AdamW flagged={flagged} clip={clip_on}: worst |device - torch| = {worst:.3e}")
    keep = pad_mask()
    for a in (p, m, v):
        assert bool((a.cpu()[~keep] == 0).all()), "a padding float moved"
    assert not torch.equal(p.cpu(), p0)
    tab.close()


# ---- 2. LAMB against the float64 definition ---------------------------------------------------------
@CASES
@FLAGGED
def test_lamb_matches_the_float64_definition(flagged, clip_on, gscale):
    L = _L()
    flags = make_flags(flagged)
    trust_clip = 0.5 if (flagged and not clip_on) else 0.0
    tab = Table(SIZES, flags)
    p0, m0, v0 = make_state(2, zero_moments=True)
    (p, cp), (m, cm), (v, cv) = gbuf(p0, "params"), gbuf(m0, "exp_avg"), gbuf(v0, "exp_avg_sq")
    clip = torch.tensor([2.0, 0.5], device="cuda") if clip_on else None
    gs = Q.gscale32(0.5 if clip_on else None, gscale)
    floors = dict(p=0.0, m=0.0, v=0.0)
    errs = dict(p=0.0, m=0.0, v=0.0)
    r_lo, r_hi, r_rel, r32_rel = float("inf"), 0.0, 0.0, 0.0
    for t in range(1, 6):
        g_cpu = make_grad(t)
        g = g_cpu.cuda()
        pre = [a.cpu() for a in (p, m, v)]
        const = Inputs(grads=g, clip_out2=clip)
        steps = (GROUP_STEP0[0] + t - 1, GROUP_STEP0[1] + t - 1)
        L.check(dev_step(Q.LAMB, tab, 0, NSEG, p, g, m, v, groups_for(0, NSEG, steps), clip, gscale,
                         trust_clip))
        cp(), cm(), cv(), tab.check(), const.check()
        got = [a.cpu() for a in (p, m, v)]
        ratios = tab.ratios.cpu()
        for s in range(NSEG):
            sl = slice(STARTS[s], ENDS[s])
            gi = group_of(s)
            kw = dict(lr=GROUP_LR[gi], step=steps[gi], gs=gs, flags=flags[s], trust_clip=trust_clip,
                      **HP)
            w64 = Q.step64(Q.LAMB, pre[0][sl], g_cpu[sl], pre[1][sl], pre[2][sl], **kw)
            w32 = Q.step32(Q.LAMB, pre[0][sl], g_cpu[sl], pre[1][sl], pre[2][sl], **kw)
            r = float(ratios[s])
            assert abs(r - w64[3]) <= 1e-6 * w64[3], \
                f"step {t} segment {s}: trust ratio {r!r} against float64 {w64[3]!r}"
            r_rel = max(r_rel, abs(r - w64[3]) / w64[3])
            r32_rel = max(r32_rel, abs(w32[3] - w64[3]) / w64[3])
            # degenerate norms: nu == 0 on every step; np == 0 on the first one (p moves from there on)
            if flags[s] & Q.NO_ADAPT or s == G0_SEG or (s == P0_SEG and t == 1):
                assert r == 1.0
            else:
                r_lo, r_hi = min(r_lo, r), max(r_hi, r)
            for j, key in enumerate(("p", "m", "v")):
                err, own = Q.gate(f"step {t} segment {s} {key}", got[j][sl], w64[j], w32[j])
                floors[key], errs[key] = max(floors[key], own), max(errs[key], err)
        g0 = slice(STARTS[G0_SEG], ENDS[G0_SEG])
        assert torch.equal(got[0][g0].view(torch.int32), p0[g0].view(torch.int32)), \
            "the nu == 0 segment's parameters moved"
    print(f"LAMB flagged={flagged} clip={clip_on} trust_clip={trust_clip}: ratios in [{r_lo:.4f}, "
          f"{r_hi:.4f}], worst relative ratio error device {r_rel:.2e} / fp32 statement {r32_rel:.2e}; "
          f"fp32-statement floors p {floors['p']:.2e} m {floors['m']:.2e} v {floors['v']:.2e}; "
          f"device errors p {errs['p']:.2e} m {errs['m']:.2e} v {errs['v']:.2e}")
    keep = pad_mask()
    for a in (p, m, v):
        assert bool((a.cpu()[~keep] == 0).all()), "a padding float moved"
    assert not torch.equal(p.cpu(), p0)
    tab.close()


# ---- 3. position independence -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", [Q.ADAMW, Q.LAMB], ids=["adamw", "lamb"])
def test_position_independence_bit_for_bit(kind):
    L = _L()
    flags = make_flags(True)
    tab = Table(SIZES, flags)
    p0, m0, v0 = make_state(3, zero_moments=False)
    g_cpu = make_grad(2)
    g = g_cpu.cuda()
    steps = (3, 7)
    clip = torch.tensor([2.0, 0.5], device="cuda")
    lamb = kind == Q.LAMB

    def run(runs):
        (p, cp), (m, cm), (v, cv) = gbuf(p0, "params"), gbuf(m0, "exp_avg"), gbuf(v0, "exp_avg_sq")
        tab.ratios.fill_(float("nan"))
        for first, count in runs:
            L.check(dev_step(kind, tab, first, count, p, g, m, v, groups_for(first, count, steps),
                             clip, 0.5))
        cp(), cm(), cv(), tab.check()
        return p.cpu(), m.cpu(), v.cpu(), tab.ratios.cpu()

    def same(a, b, what, sl=slice(None)):
        for name, x, y in zip(("p", "exp_avg", "exp_avg_sq"), a, b):
            assert torch.equal(x[sl].view(torch.int32), y[sl].view(torch.int32)), f"{what}: {name}"
        if lamb:
            assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32)), f"{what}: ratios"

    whole = run([(0, NSEG)])
    assert not torch.equal(whole[0], p0)
    if lamb:
        assert bool(torch.isfinite(whole[3]).all())
    same(run([(0, NSEG)]), whole, "two identical runs")
    same(run([(0, 30), (30, NSEG - 30)]), whole, "split at a segment boundary")
    same(run([(46, 3), (0, 46)]), whole, "split, later run first")
    # a run inside the table: the rest is untouched
    part = run([(10, 30)])
    inside = slice(STARTS[10], ENDS[39])
    for j, (name, init) in enumerate((("p", p0), ("exp_avg", m0), ("exp_avg_sq", v0))):
        assert torch.equal(part[j][inside], whole[j][inside]), f"run [10, 40): {name} inside"
        for out in (slice(0, STARTS[10]), slice(ENDS[39], N)):
            assert torch.equal(part[j][out].view(torch.int32), init[out].view(torch.int32)), \
                f"run [10, 40): {name} outside the run was written"
    if lamb:
        assert torch.equal(part[3][10:40], whole[3][10:40])
        assert bool(torch.isnan(part[3][:10]).all()) and bool(torch.isnan(part[3][40:]).all())
    # single segments in allocations and tables of their own
    for s in (2, 46, 43, G0_SEG, P0_SEG, 47, 48):
        sl = slice(STARTS[s], ENDS[s])
        one = Table([SIZES[s]], [flags[s]])
        (p, cp), (m, cm), (v, cv) = gbuf(p0[sl], "params"), gbuf(m0[sl], "exp_avg"), gbuf(v0[sl], "exp_avg_sq")
        gi = group_of(s)
        L.check(dev_step(kind, one, 0, 1, p, g_cpu[sl].cuda(), m, v,
                         [(SIZES[s], GROUP_LR[gi], steps[gi])], clip, 0.5))
        cp(), cm(), cv(), one.check()
        for j, x in enumerate((p, m, v)):
            assert torch.equal(x.cpu().view(torch.int32), whole[j][sl].view(torch.int32)), \
                f"segment {s} alone differs from the same segment inside the table (array {j})"
        if lamb:
            assert torch.equal(one.ratios.cpu().view(torch.int32), whole[3][s:s + 1].view(torch.int32))
        one.close()
    keep = pad_mask()
    for a in whole[:3]:
        assert bool((a[~keep] == 0).all()), "a padding float moved"
    tab.close()


# ---- 4. refusals: non-zero, a message that names the argument, nothing launched --------------------
def _refused(rc, needle):
    assert rc != 0
    msg = (_L().lib().cilrs_last_error() or b"").decode()
    assert needle in msg, msg


def test_refusals_happen_before_any_launch():
    L = _L()
    lib = L.lib()
    # the table entry
    mem, check_mem = guarded(4096, dtype=torch.uint8, fill=None, name="table")
    before = mem.clone()

    def create(ends, flags, n, ptr=None, nbytes=4096):
        k = len(ends)
        h = C.c_void_p(1)
        rc = lib.cilrs_optim_table_create((C.c_size_t * k)(*ends), (C.c_int * k)(*flags), k, n,
                                          L.ptr(mem) if ptr is None else ptr, nbytes, stream(),
                                          C.byref(h))
        assert rc == 0 or not h.value
        return rc

    _refused(create([4, 10, 16], [0, 0, 0], 16), "multiple of 4")
    _refused(create([8, 8, 16], [0, 0, 0], 16), "increase")
    _refused(create([8, 4, 16], [0, 0, 0], 16), "increase")
    _refused(create([8, 16], [0, 0], 20), "last end")
    _refused(create([8, 16], [0, 4], 16), "flags")
    _refused(create([8, 16], [0, 0], 16, ptr=C.c_void_p(0)), "device_table")
    _refused(create([8, 16], [0, 0], 16, ptr=C.c_void_p(mem.data_ptr() + 4)), "aligned")
    _refused(create([8, 16], [0, 0], 16, nbytes=48), "device_bytes")
    check_mem()
    assert torch.equal(mem, before), "a refused table build wrote the device table"
    # the step entry
    tab = Table(SIZES, make_flags(True))
    cpu = dict(zip(("p", "m", "v"), make_state(4, zero_moments=False)))
    cpu["g"] = make_grad(1)
    bufs = {k: gbuf(t, k) for k, t in cpu.items()}
    p, m, v, g = (bufs[k][0] for k in ("p", "m", "v", "g"))
    ok = groups_for(0, NSEG, (1, 4))

    def step(kind=Q.LAMB, first=0, count=NSEG, groups=ok, P=p, G=g, M=m, V=v, **kw):
        return dev_step(kind, tab, first, count, P, G, M, V, groups, **kw)

    for kind in (Q.ADAMW, Q.LAMB):
        _refused(step(kind, groups=[(ENDS[GROUP_SPLIT - 1] + 8, 1e-3, 1), (N, 1e-3, 1)]), "group_ends")
        _refused(step(kind, groups=[(N - 4, 1e-3, 1)]), "group")
        _refused(step(kind, groups=[(ENDS[3], 1e-3, 1), (ENDS[3], 1e-3, 1), (N, 1e-3, 1)]), "group_ends")
        _refused(step(kind, groups=[(N, 1e-3, 0)]), "step")
        _refused(step(kind, groups=[(ENDS[9], 1e-3, 3), (N, 1e-3, -2)]), "step")
        _refused(step(kind, table=None), "table")
        _refused(step(kind, P=p[1:]), "aligned")
        _refused(step(kind, G=g[2:]), "aligned")
        _refused(step(kind, M=m[1:]), "aligned")
        _refused(step(kind, V=v[3:]), "aligned")
        _refused(step(kind, first=-1), "first_seg")
        _refused(step(kind, first=40, count=NSEG - 39), "first_seg")
        _refused(step(kind, count=0), "count")
        _refused(step(kind, groups=ok * 5), "ngroups")
        _refused(step(kind, trust_clip=-1.0), "trust_clip")
    _refused(step(3), "kind")
    _refused(step(Q.LAMB, scratch=None), "scratch")
    _refused(step(Q.LAMB, scratch=C.c_void_p(tab.scratch.data_ptr() + 4)), "scratch")
    _refused(L.lib().cilrs_optim_step(Q.LAMB, tab.h, 0, NSEG, None, L.ptr(g), L.ptr(m), L.ptr(v), 1,
                                      (C.c_size_t * 1)(N), (C.c_double * 1)(1e-3), (C.c_int64 * 1)(1),
                                      0.9, 0.999, 1e-6, 0.0, 0.0, None, 1.0, L.ptr(tab.scratch), None,
                                      stream()), "NULL")
    tab.check()
    for k, (t, check) in bufs.items():
        check()
        assert torch.equal(t.cpu().view(torch.int32), cpu[k].view(torch.int32)), f"{k} was written"
    assert bool(torch.isnan(tab.ratios).all()), "ratio_out was written by a refused call"
    tab.close()


# ====================================================================================================
# Trainer level: B = 8 synthetic batches, portable weights
# ====================================================================================================
@pytest.fixture(scope="module")
def weights():
    from cilrs_mi355 import CILRS
    return O.portable_state_dict(CILRS(4, 0.0).state_dict(), 0)


def make_model(weights):
    from cilrs_mi355 import CILRS
    m = CILRS(num_commands=4, dropout=0.0)
    m.load_state_dict(weights, strict=True)
    return m.cuda()


def batches(k, seed0=70):
    return [[t.cuda() for t in O.synthetic_batch(8, seed=seed0 + i)[:4]] for i in range(k)]


def cfg_with(base, **kw):
    from cilrs_mi355 import TrainConfig
    return TrainConfig(**{**base.__dict__, **kw})


def snapshot(tr):
    return dict(params=tr.eng.params.cpu(), exp_avg=tr.exp_avg.cpu(), exp_avg_sq=tr.exp_avg_sq.cpu())


def check_one_step(tr, before, frozen_groups=0):
    """The step just taken, tensor by tensor through tests/_optim.py on the CPU, from the gradients
    the arena still holds.  LAMB: the rule of _optim.gate and the ratio within 1e-6 of float64;
    AdamW: 1e-6 element-wise against the fp32 statement."""
    from cilrs_mi355.train import segment_table
    eng, cfg = tr.eng, tr.cfg
    lamb = cfg.optimizer == "lamb"
    kind = Q.LAMB if lamb else Q.ADAMW
    ends, flags = segment_table(eng.params_layout, eng.n_arena, cfg.decay_exempt_1d, lamb)
    after = snapshot(tr)
    g = eng.grads.cpu()
    coef = float(tr.clip_out[1]) if cfg.grad_clip > 0 else None
    gs = Q.gscale32(coef, 1.0 if coef is not None else tr.arena_grad_scale)
    begin = eng.trainable_begin(frozen_groups)
    steps = tr.group_steps
    ratios = tr.trust_ratios() if lamb else None
    assert ratios is None or tuple(ratios.shape) == (len(eng.params_layout),)
    keys = ("params", "exp_avg", "exp_avg_sq")
    worst = dict.fromkeys(keys, 0.0)
    floors = dict.fromkeys(keys, 0.0)
    for i, (name, off, numel, _) in enumerate(eng.params_layout):
        sl = slice(off, ends[i])
        if off < begin:
            for k in keys:
                assert torch.equal(after[k][sl], before[k][sl]), f"frozen {name}: {k} moved"
            continue
        gi = next(j for j, (b, e) in enumerate(eng.group_ranges) if b <= off < e)
        kw = dict(lr=tr.lr_now * tr.lr_mult[gi], step=steps[gi], b1=cfg.betas[0], b2=cfg.betas[1],
                  eps=cfg.eps, wd=cfg.weight_decay, gs=gs, flags=flags[i], trust_clip=cfg.trust_clip)
        args = (before["params"][sl], g[sl], before["exp_avg"][sl], before["exp_avg_sq"][sl])
        w32 = Q.step32(kind, *args, **kw)
        if not lamb:
            for j, k in enumerate(keys):
                err = float((after[k][sl] - w32[j]).abs().max())
                worst[k] = max(worst[k], err)
                assert err <= 1e-6, f"{name}: {k} differs from the fp32 statement by {err:.3e}"
            continue
        w64 = Q.step64(kind, *args, **kw)
        r = float(ratios[i])
        assert abs(r - w64[3]) <= 1e-6 * w64[3], f"{name}: trust ratio {r!r} vs float64 {w64[3]!r}"
        if flags[i] & Q.NO_ADAPT:
            assert r == 1.0
        for j, k in enumerate(keys):
            err, own = Q.gate(f"{name} {k}", after[k][sl], w64[j], w32[j])
            worst[k], floors[k] = max(worst[k], err), max(floors[k], own)
    assert not torch.equal(after["params"][begin:], before["params"][begin:])
    print(f"{cfg.optimizer}: worst errors {worst}, fp32-statement floors {floors}")


ONE_STEP = {
    "lamb": (dict(optimizer="lamb"), None),
    "lamb-exempt-clip-mult": (dict(optimizer="lamb", decay_exempt_1d=True, grad_clip=1.0,
                                   lr_mult={"stem": 0.1}), None),
    "lamb-frozen": (dict(optimizer="lamb"), "layer1"),
    "adamw-exempt": (dict(optimizer="adamw", decay_exempt_1d=True), None),
}


@pytest.mark.parametrize("case", list(ONE_STEP))
def test_trainer_one_step_is_the_definition(weights, case):
    from cilrs_mi355 import CONFIG_A, Trainer
    kw, freeze = ONE_STEP[case]
    m = make_model(weights)
    tr = Trainer(m, cfg_with(CONFIG_A, **kw))
    frozen = 0
    data = batches(2)
    if freeze is not None:
        tr.train_step(*data[0])                      # one step with everything trainable first
        m.train()
        m.freeze(freeze)
        frozen = 2                                   # stem and layer1
    before = snapshot(tr)
    tr.train_step(*data[1])
    torch.cuda.synchronize()
    if freeze is not None:
        assert tr.group_steps == [1, 1, 2, 2, 2, 2] and tr.eng.trainable_begin(frozen) > 0
    if tr.cfg.optimizer == "adamw":
        with pytest.raises(RuntimeError, match="lamb"):
            tr.trust_ratios()
    check_one_step(tr, before, frozen)


def test_adam_with_every_new_field_at_its_default_is_the_parents_step(weights):
    from cilrs_mi355 import CONFIG_A, TrainConfig, Trainer
    spelled = cfg_with(CONFIG_A, optimizer="adam", decay_exempt_1d=False, trust_clip=0.0,
                       warmup_steps=0, lr_schedule="step")
    assert spelled == TrainConfig()
    data = batches(2)
    out = []
    for cfg in (CONFIG_A, spelled):
        tr = Trainer(make_model(weights), cfg)
        assert tr._optim_table is None and tr.lr_now == tr.lr == cfg.lr
        for b in data:
            tr.train_step(*b)
        out.append(snapshot(tr))
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k


# ---- 6. data parallel, world size 1 -----------------------------------------------------------------
def test_data_parallel_bucket_route_equals_the_arena_route(weights, tmp_path):
    import torch.distributed as dist
    from cilrs_mi355 import CONFIG_A, Trainer
    cfg = cfg_with(CONFIG_A, optimizer="lamb", decay_exempt_1d=True, warmup_steps=2)
    data = batches(2)
    out = {}
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        for bucket in (True, False):
            tr = Trainer(make_model(weights), cfg, process_group=dist.group.WORLD)
            tr.bucket_optimizer = bucket
            for b in data:
                tr.train_step(*b)
            torch.cuda.synchronize()
            assert tr.step_count == 2
            out[bucket] = (snapshot(tr), tr.trust_ratios())
    finally:
        dist.destroy_process_group()
    for k in out[True][0]:
        assert torch.equal(out[True][0][k], out[False][0][k]), f"{k}: per-bucket LAMB != arena LAMB"
    assert torch.equal(out[True][1], out[False][1])
    single = Trainer(make_model(weights), cfg)
    for b in data:
        single.train_step(*b)
    assert torch.equal(single.eng.params.cpu(), out[True][0]["params"])


# ---- 7. EMA behind the LAMB step ---------------------------------------------------------------------
def test_ema_follows_the_lamb_step_and_the_fused_routes_are_refused(weights):
    from cilrs_mi355 import CONFIG_A, Trainer
    tr = Trainer(make_model(weights), cfg_with(CONFIG_A, optimizer="lamb", ema_decay=0.9,
                                               ema_warmup=True))
    ema = tr.eng.params.cpu()
    data = batches(2)
    for t, b in enumerate(data, 1):
        tr.train_step(*b)
        ema = E.step32(ema, tr.eng.params.cpu(), E.weight32(0.9, t, True))
        assert tr.ema_updates == t and torch.equal(tr.ema.cpu(), ema), f"update {t}"
    assert not torch.equal(tr.ema, tr.eng.params)
    state = (snapshot(tr), tr.ema.clone(), tr.eng.grads.clone())
    for attr in ("ema_fused", "fuse_optimizer"):
        setattr(tr, attr, True)
        with pytest.raises(RuntimeError, match=attr):
            tr.train_step(*data[0])
        with pytest.raises(RuntimeError, match=attr):
            tr.optimizer_step()
        setattr(tr, attr, False)
    torch.cuda.synchronize()
    now = snapshot(tr)
    assert all(torch.equal(now[k], state[0][k]) for k in now) and torch.equal(tr.ema, state[1])
    assert torch.equal(tr.eng.grads, state[2]) and tr.step_count == 2 and tr.ema_updates == 2


# ---- 8. fit, checkpoints, resume ---------------------------------------------------------------------
CONFIG_KEYS = {"name", "lr", "weight_decay", "loss", "loss_weights", "grad_clip", "dropout", "betas",
               "eps", "lr_step_size", "lr_gamma", "lr_mult"}
NEW = dict(optimizer="lamb", warmup_steps=3, lr_schedule="cosine", lr_epochs=3, lr_min=1e-5)


def _fit(weights, out_dir, epochs, resume=None, **kw):
    from cilrs_mi355 import CONFIG_A, Trainer
    from cilrs_mi355.loop import fit
    m = make_model(weights)
    tr = Trainer(m, cfg_with(CONFIG_A, **kw))
    train, val = batches(2, seed0=70), batches(1, seed0=20)
    rates = []
    res = fit(tr, lambda: train, lambda: val, epochs=epochs, patience=6, out_dir=str(out_dir),
              resume=resume, log=lambda line: rates.append((tr.lr, tr.lr_now)))
    return tr, res


def test_fit_round_trip_with_warmup_and_cosine(weights, tmp_path):
    from cilrs_mi355 import CONFIG_A
    from cilrs_mi355.checkpoint import load_file
    from cilrs_mi355.train import cosine_lr
    tr, _ = _fit(weights, tmp_path / "a", 2, **NEW)
    cfg = tr.cfg
    assert tr.step_count == 4 and tr.epoch == 2
    assert tr.lr == cosine_lr(cfg, 2) == tr.lr_now           # the warm-up is over after step 3
    latest = load_file(tmp_path / "a" / "checkpoint_latest.pth")
    best = load_file(tmp_path / "a" / "checkpoint_best.pth")
    for ck in (latest, best):
        assert set(ck["config"]) == CONFIG_KEYS | set(NEW)
        assert {k: ck["config"][k] for k in NEW} == NEW
    assert set(latest["optimizer_state_dict"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    resumed, _ = _fit(weights, tmp_path / "b", 3, resume=str(tmp_path / "a" / "checkpoint_latest.pth"),
                      **NEW)
    whole, _ = _fit(weights, tmp_path / "c", 3, **NEW)
    assert resumed.step_count == whole.step_count == 6 and resumed.lr == whole.lr == 1e-5
    assert torch.equal(resumed.eng.params, whole.eng.params)
    assert torch.equal(resumed.exp_avg, whole.exp_avg)
    assert torch.equal(resumed.exp_avg_sq, whole.exp_avg_sq)
    assert torch.equal(resumed.trust_ratios(), whole.trust_ratios())
    # the same file into an Adam trainer: refused, and the other way round
    with pytest.raises(ValueError, match="optimizer"):
        _fit(weights, tmp_path / "d", 3, resume=str(tmp_path / "a" / "checkpoint_latest.pth"))
    adam, _ = _fit(weights, tmp_path / "e", 1)
    assert set(load_file(tmp_path / "e" / "checkpoint_best.pth")["config"]) == CONFIG_KEYS
    assert "config" not in load_file(tmp_path / "e" / "checkpoint_latest.pth")
    with pytest.raises(ValueError, match="optimizer"):
        _fit(weights, tmp_path / "f", 2, resume=str(tmp_path / "e" / "checkpoint_latest.pth"), **NEW)
