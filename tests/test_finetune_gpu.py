"""Fine-tuning with a frozen trunk prefix (CILRS.freeze / torch's own idiom) against the CPU oracle
driven with the same torch calls: forward, backward, clip, Adam, checkpoints, data parallel.

``oracle.train_step`` calls ``model.train()``, which undoes a per-module ``.eval()``, so this file
has its own six-line step (_ostep).  ``portable_state_dict`` leaves the running statistics at 0 / 1:
every test starts from a state two full oracle steps later (_warm_state), loaded into both models --
otherwise a frozen BatchNorm is indistinguishable from none.

Tolerances are the project's existing ones (tests/test_model_gpu.py): outputs and
losses 1e-4, running statistics 1e-5, per-tensor gradient error against a float64 run <= max(4x the
fp32 CPU oracle's, 5e-3), clip norm 5e-4 relative, parameters after Adam through _close_params,
Winograd op 5e-5 of max|ref|, Adam op 1e-6.
"""
import copy
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import cilrs_oracle as O
from test_model_gpu import _cfgs, _close_params, _grad_views, to_dev

pytestmark = pytest.mark.gpu

GROUPS = ("stem", "layer1", "layer2", "layer3", "layer4")
N_CHILDREN = {1: 4, 2: 5, 3: 6, 4: 7, 5: 8}          # visual_encoder[:n] = the first k groups


# ---- helpers -------------------------------------------------------------------------------------
def _builders(variant):
    if variant == 1:
        import resnet50_oracle as R
        from cilrs_mi355 import CILRSResNet50
        return R.build_oracle50, CILRSResNet50
    from cilrs_mi355 import CILRS
    return O.build_oracle, CILRS


@functools.lru_cache(maxsize=None)
def _warm_state(cfg_name="A", variant=0, batch=8):
    """state_dict of the oracle after two full train steps (running statistics moved)."""
    _, ocfg = _cfgs()[cfg_name]
    build, _ = _builders(variant)
    orc = build(0)
    opt = O.make_optimizer(orc, ocfg)
    for s in range(2):
        O.train_step(orc, opt, ocfg, *O.synthetic_batch(batch, seed=900 + s)[:4])
    return {k: v.detach().clone() for k, v in orc.state_dict().items()}


def _pair(cfg_name="A", variant=0, batch=8):
    """(HIP model on the GPU, oracle), both in train mode, both in the warm state."""
    build, cls = _builders(variant)
    sd = _warm_state(cfg_name, variant, batch)
    orc = build(0)
    orc.load_state_dict(sd, strict=True)
    m = cls(4, 0.0)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train(), orc.train()


def _idiom(model, k, bn_eval=True):
    """torch's usual idiom, the same calls on either model."""
    prefix = model.visual_encoder[:N_CHILDREN[k]]
    if bn_eval:
        prefix.eval()
    for p in prefix.parameters():
        p.requires_grad_(False)


def _prefix_keys(sd, k):
    heads = tuple(f"visual_encoder.{i}." for i in range(N_CHILDREN[k]))
    return [n for n in sd if n.startswith(heads)]


def _ostep(orc, opt, ocfg, imgs, spds, cmds, tgts):
    """forward, compute_loss, backward, clip, optimizer.step -- without model.train()."""
    pc, ps = orc(imgs, spds, cmds)
    loss, ld = O.compute_loss(ocfg, pc, tgts, ps, spds)
    opt.zero_grad()
    loss.backward()
    live = [p for p in orc.parameters() if p.grad is not None]
    gn = float(torch.nn.utils.clip_grad_norm_(live, ocfg.grad_clip)) if ocfg.grad_clip > 0 else None
    opt.step()
    return ld, gn


def _fp64(orc, ocfg, k, bn_eval, batch):
    """Gradients of the same step in float64, from a copy of `orc` (flags included)."""
    m64 = copy.deepcopy(orc).double()
    imgs, spds, cmds, tgts = batch
    pc, ps = m64(imgs.double(), spds.double(), cmds)
    loss, _ = O.compute_loss(ocfg, pc, tgts.double(), ps, spds.double())
    loss.backward()
    return {n: p.grad for n, p in m64.named_parameters()}


def _snapshot(m, tr, names):
    sd = m.state_dict()
    eng = tr.eng
    snap = {n: sd[n].detach().clone() for n in names}
    cut = None
    for (n, off, numel, _), in zip(eng.params_layout):
        if n not in snap:
            cut = off
            break
    snap["__m"] = tr.exp_avg[:cut].clone()
    snap["__v"] = tr.exp_avg_sq[:cut].clone()
    snap["__cut"] = cut
    return snap


def _assert_frozen_untouched(m, tr, snap):
    sd = m.state_dict()
    for n, v in snap.items():
        if n.startswith("__"):
            continue
        assert torch.equal(sd[n], v), f"frozen {n} moved"
    cut = snap["__cut"]
    assert torch.equal(tr.exp_avg[:cut], snap["__m"]) and torch.equal(tr.exp_avg_sq[:cut], snap["__v"])


def _check_step(m, tr, orc, opt, cfg, ocfg, k, bn_eval, seed, batch_size=8, outputs=True,
                ltol=1e-4, param_steps=1):
    """One fine-tuning step on both sides + every gate of test 1 (or, bn_eval=False, test 2)."""
    batch = O.synthetic_batch(batch_size, seed=seed)[:4]
    imgs, spds, cmds, tgts = batch
    dbatch = to_dev(*batch)
    sd0 = {n: v.detach().clone() for n, v in m.state_dict().items()}
    frozen = _prefix_keys(sd0, k) if k else []
    if not bn_eval:      # running statistics and num_batches_tracked of the prefix follow torch's
        frozen = [n for n in frozen if "running_" not in n and "num_batches" not in n]
    snap = _snapshot(m, tr, frozen) if k else None
    if outputs:
        # train-mode outputs: one forward without a graph on both sides (moves the trainable
        # running statistics once more, on both sides alike)
        with torch.no_grad():
            pc, ps = m(*dbatch[:3])
            opc, ops = orc(imgs, spds, cmds)
        eo = max(float((pc.cpu() - opc).abs().max()), float((ps.cpu() - ops).abs().max()))
        print(f"k={k} train-mode outputs err {eo:.2e}")
        assert eo <= 1e-4
    g64 = _fp64(orc, ocfg, k, bn_eval, batch)
    tr.train_step(*dbatch)
    got = tr.losses()
    old, ogn = _ostep(orc, opt, ocfg, imgs, spds, cmds, tgts)
    for key, v in old.items():
        print(f"k={k} loss {key}: {got[key]:.6f} vs {v:.6f}")
        assert abs(got[key] - v) <= ltol * max(1.0, abs(v)), (key, got[key], v)
    if k:
        _assert_frozen_untouched(m, tr, snap)
    # running statistics that move: 1e-5
    sd = m.state_dict()
    osd = orc.state_dict()
    for n in sd:
        if "running_" in n and n not in frozen:
            err = float((sd[n].cpu() - osd[n]).abs().max())
            assert err <= 1e-5 * max(1.0, float(osd[n].abs().max())), (n, err)
        if n.endswith("num_batches_tracked"):
            assert int(sd[n]) == int(osd[n]), n
    # gradients: trainable tensors only; frozen ones have none on the oracle side
    gv = _grad_views(tr.eng)
    coef = 1.0
    live64 = {n: g for n, g in g64.items() if g is not None}
    n_live = sum(1 for p in orc.parameters() if p.grad is not None)
    assert len(live64) == n_live
    if cfg.grad_clip > 0:
        gn64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in live64.values())))
        gn = tr.grad_norm()
        print(f"k={k} clip norm {gn:.6f} vs float64 {gn64:.6f} (oracle fp32 {ogn:.6f})")
        assert abs(gn - gn64) <= 5e-4 * gn64
        coef = min(1.0, cfg.grad_clip / (gn64 + 1e-6))
    worst = (0.0, 0.0, "")
    for n, p in orc.named_parameters():
        if p.grad is None:
            assert n not in live64
            continue
        ref64 = live64[n] * coef
        nrm = max(float(ref64.norm()), 1e-30)
        e_gpu = float((gv[n].detach().cpu().double() * coef - ref64).norm()) / nrm
        e_cpu = float((p.grad.double() - ref64).norm()) / nrm
        if e_gpu > worst[0]:
            worst = (e_gpu, e_cpu, n)
        assert e_gpu <= max(4.0 * e_cpu, 5e-3), (n, e_gpu, e_cpu)
    print(f"k={k} worst per-tensor gradient error vs float64: HIP {worst[0]:.2e} "
          f"(CPU fp32 {worst[1]:.2e}) on {worst[2]}; {n_live} gradient tensors")
    pv = dict(m.named_parameters())
    for n, p in orc.named_parameters():
        if p.grad is not None:
            _close_params(pv[n].detach().cpu(), p.detach(), cfg.lr, param_steps)
    return n_live


# ---- 1. step against the oracle, e == g == k -------------------------------------------------------
# The batch.  At B = 8 every fp32 implementation takes a few of the ~3 M trunk ReLU decisions of a
# step differently from a float64 run -- units whose pre-activation lies within rounding of zero --
# and each such decision moves every gradient tensor upstream of it by 1e-3 .. 1e-2 relative (one
# unit is 1 / 624 of a layer3 channel's pixels).  Measured on MI355X over k = 1..4 x Config A, B x
# seeds 40..45 (48 steps, against float64): the HIP engine differs on 0..6 decisions per step, the
# fp32 CPU oracle on 0..5, the largest activation on any such unit is 4.2e-6 on the engine's side
# and 3.6e-6 on the oracle's; on the steps where neither side differs (eight of them) the worst
# tensor of the engine is 1.0e-6 .. 1.2e-6 from float64, the oracle's 0.9e-6 .. 1.1e-6.  The gate
# max(4x the oracle's error, 5e-3) holds on 38 of the 48 steps and is missed on 10 (1 .. 9 tensors),
# each time because the engine's rounding-level decisions hit harder than the oracle's on that
# batch; by the same luck the oracle is the worse of the two on 9 other steps (median tensor up to
# 1.4e-3 against the engine's 1e-6).  One seed for all ten cases, the first of the scan:
STEP_SEED = 40
@pytest.mark.parametrize("cfg_name", ["A", "B"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_frozen_prefix_step_matches_oracle(k, cfg_name):
    """Fails on a code base without the feature: the frozen tensors move there."""
    from cilrs_mi355 import Trainer
    cfg, ocfg = _cfgs()[cfg_name]
    m, orc = _pair(cfg_name)
    _idiom(m, k)
    _idiom(orc, k)
    assert m.freeze_state() == (k, k)
    tr = Trainer(m, cfg)
    opt = O.make_optimizer(orc, ocfg)
    n_live = _check_step(m, tr, orc, opt, cfg, ocfg, k, True, seed=STEP_SEED)
    assert len(_prefix_keys(m.state_dict(), k)) == {1: 6, 2: 42, 3: 96, 4: 174, 5: 216}[k]
    assert n_live == {1: 139, 2: 121, 3: 94, 4: 55, 5: 34}[k]


# ---- 2. requires_grad only: e == 0 -------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5])
def test_requires_grad_only_keeps_batch_statistics_in_the_prefix(k):
    from cilrs_mi355 import Trainer
    cfg, ocfg = _cfgs()["B"]
    m, orc = _pair("B")
    _idiom(m, k, bn_eval=False)
    _idiom(orc, k, bn_eval=False)
    assert m.freeze_state() == (0, k)
    nbt0 = int(m.state_dict()["visual_encoder.1.num_batches_tracked"])
    tr = Trainer(m, cfg)
    opt = O.make_optimizer(orc, ocfg)
    _check_step(m, tr, orc, opt, cfg, ocfg, k, False, seed=41 + k)
    assert int(m.state_dict()["visual_encoder.1.num_batches_tracked"]) == nbt0 + 2   # forward + step


# ---- 3. launch accounting ------------------------------------------------------------------------------
def _profiled_step(m, tr, dbatch):
    pl = tr.eng.plan(dbatch[0].size(0), dbatch[0].size(2), dbatch[0].size(3))
    pl.profile(True)
    try:
        pl.profile_reset()
        tr.train_step(*dbatch)
        torch.cuda.synchronize()
        # (labels seen by an earlier window stay in the table with zero calls)
        return {k: v for k, v in pl.profile_table().items() if v["calls"] > 0}
    finally:
        pl.profile(False)


def test_no_launch_carries_a_frozen_groups_label():
    from cilrs_mi355 import Trainer
    cfg, _ = _cfgs()["A"]
    m, _ = _pair("A")
    tr = Trainer(m, cfg)
    dbatch = to_dev(*O.synthetic_batch(8, seed=51)[:4])
    tr.train_step(*dbatch)                                  # plan built outside the window
    full = _profiled_step(m, tr, dbatch)
    m.freeze("layer1")                                     # k = 2
    tr.train_step(*dbatch)
    cut = _profiled_step(m, tr, dbatch)
    m.unfreeze()
    again = _profiled_step(m, tr, dbatch)
    for kind in ("bn_fwd", "bn_bwd", "conv_dgrad", "conv_wgrad"):
        for grp in ("stem", "layer1"):
            assert f"{kind}.{grp}" not in cut, (kind, grp)
            assert f"{kind}.{grp}" in full or (kind, grp) == ("conv_dgrad", "stem")
    # layer2 is the last trainable group: its first block launches no data gradient into layer1
    # (conv1's and the down-sample's), everything else of the group is there
    assert cut["conv_dgrad.layer2"]["calls"] == full["conv_dgrad.layer2"]["calls"] - 2
    for kind in ("bn_fwd", "bn_bwd", "conv_wgrad", "conv_fwd"):
        assert cut[f"{kind}.layer2"]["calls"] == full[f"{kind}.layer2"]["calls"], kind
    for grp in ("layer3", "layer4"):
        for kind in ("bn_fwd", "bn_bwd", "conv_dgrad", "conv_wgrad", "conv_fwd"):
            assert cut[f"{kind}.{grp}"]["calls"] == full[f"{kind}.{grp}"]["calls"], (kind, grp)
    assert "maxpool" in cut and cut["conv_fwd.stem"]["calls"] == 1
    # k = 0 keeps the full step's counts, label by label
    assert {k_: v["calls"] for k_, v in again.items()} == {k_: v["calls"] for k_, v in full.items()}


def test_no_launch_carries_a_frozen_groups_label_layer3_boundary():
    """The same with layer3 as the last trainable group (freeze("layer2")): no bn_fwd / bn_bwd /
    conv_dgrad / conv_wgrad entry labelled stem, layer1 or layer2, and layer3 short of exactly
    the two boundary launches."""
    from cilrs_mi355 import Trainer
    cfg, _ = _cfgs()["A"]
    m, _ = _pair("A")
    tr = Trainer(m, cfg)
    dbatch = to_dev(*O.synthetic_batch(8, seed=52)[:4])
    tr.train_step(*dbatch)
    full = _profiled_step(m, tr, dbatch)
    m.freeze("layer2")
    tr.train_step(*dbatch)
    cut = _profiled_step(m, tr, dbatch)
    for kind in ("bn_fwd", "bn_bwd", "conv_dgrad", "conv_wgrad"):
        for grp in ("stem", "layer1", "layer2"):
            assert f"{kind}.{grp}" not in cut, (kind, grp)
    assert cut["conv_dgrad.layer3"]["calls"] == full["conv_dgrad.layer3"]["calls"] - 2
    for kind in ("bn_fwd", "bn_bwd", "conv_wgrad"):
        assert cut[f"{kind}.layer3"]["calls"] == full[f"{kind}.layer3"]["calls"], kind


# ---- 4. Winograd kernel with the folded epilogue, op level -----------------------------------------------
FOLD_CASES = [
    (128, 22, 50, 64, 64),       # layer1 at the benchmark batch
    (128, 11, 25, 128, 128),     # layer2
    (128, 6, 13, 256, 256),      # layer3
    (3, 7, 9, 72, 192),          # ragged: odd sizes, Cin not a multiple of 64, a tail-only launch
]


@pytest.mark.parametrize("relu,relu_post,with_add", [(1, 0, False), (0, 1, True), (0, 0, False),
                                                     (1, 1, True)])
@pytest.mark.parametrize("case", FOLD_CASES)
def test_conv_wino_folded_epilogue(case, relu, relu_post, with_add):
    """y = relu_post?(relu?(conv * scale + shift) + addend) against torch's direct convolution and
    the affine map in float64; gate: 5e-5 of max|ref|, the Winograd op gate."""
    from cilrs_mi355 import _lib as L
    lib = L.lib()
    N, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.5
    add = torch.randn(N, Cout, H, W, generator=g)
    torch.set_num_threads(16)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if relu:
        ref = ref.clamp_min(0)
    if with_add:
        ref = ref + add.double()
    if relu_post:
        ref = ref.clamp_min(0)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    wd = w.permute(0, 2, 3, 1).contiguous().cuda()
    addd = add.permute(0, 2, 3, 1).contiguous().cuda()
    sc, sh = scale.cuda(), shift.cuda()
    y = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    scratch = torch.empty(lib.cilrs_conv2d_wino_scratch_floats(Cin, Cout), device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.cilrs_conv2d_wino_fold_fwd(L.ptr(xd), L.ptr(wd), L.ptr(y), L.ptr(sc), L.ptr(sh),
                                           L.ptr(addd) if with_add else None, relu, relu_post,
                                           N, H, W, Cin, Cout, L.ptr(scratch), s))
    torch.cuda.synchronize()
    got = y.cpu().permute(0, 3, 1, 2).double()
    assert torch.isfinite(got).all()
    err = float((got - ref).abs().max())
    print(f"{case} relu={relu} relu_post={relu_post} add={with_add}: err {err:.2e} of max "
          f"{float(ref.abs().max()):.2f}")
    assert err <= 5e-5 * max(1.0, float(ref.abs().max())), err


# ---- 5. the benchmark batch: the folded Winograd epilogue runs inside the network --------------------------
def test_b128_k3_step_and_frozen_winograd_launches():
    from cilrs_mi355 import Trainer
    cfg, ocfg = _cfgs()["A"]
    m, orc = _pair("A")
    m.freeze("layer2")
    _idiom(orc, 3)
    tr = Trainer(m, cfg)
    batch = O.synthetic_batch(128, seed=61)[:4]
    dbatch = to_dev(*batch)
    with torch.no_grad():
        pc, ps = m(*dbatch[:3])
        opc, ops = orc(*batch[:3])
    eo = max(float((pc.cpu() - opc).abs().max()), float((ps.cpu() - ops).abs().max()))
    print(f"B=128 k=3 outputs err {eo:.2e}")
    assert eo <= 1e-4
    tr.train_step(*dbatch)
    got = tr.losses()
    opt = O.make_optimizer(orc, ocfg)
    old, _ = _ostep(orc, opt, ocfg, *batch)
    for key, v in old.items():
        assert abs(got[key] - v) <= 1e-4 * max(1.0, abs(v)), (key, got[key], v)
    pl = tr.eng.last_plan
    # eligible = the train plan's own test (Plan.wino_convs counts them over layers 1-3: every
    # 3x3 / stride-1 convolution, 3 + 3 in layer1, 3 + 4 in layer2, 5 + 6 in layer3); the frozen
    # prefix holds layer1's six and layer2's seven
    assert pl.wino_convs() == 24
    assert pl.ft_wino_convs() == 13


# ---- 6. autograd path ---------------------------------------------------------------------------------------
def test_autograd_path_uses_the_same_cut():
    from cilrs_mi355 import Trainer
    cfg, ocfg = _cfgs()["A"]
    batch = O.synthetic_batch(8, seed=71)[:4]
    dbatch = to_dev(*batch)
    # Trainer path
    m1, _ = _pair("A")
    m1.freeze("layer3")
    tr = Trainer(m1, cfg)
    tr.train_step(*dbatch)
    want = {n: g.detach().clone() for n, g in _grad_views(tr.eng).items()}
    # loss.backward() + torch.optim.Adam
    m2, orc = _pair("A")
    m2.freeze("layer3")
    sd0 = {n: v.detach().clone() for n, v in m2.state_dict().items()}
    opt = torch.optim.Adam((p for p in m2.parameters() if p.requires_grad), lr=cfg.lr,
                           weight_decay=cfg.weight_decay)
    # (a) the same output gradients through autograd: bit-identical parameter gradients.  (torch's
    #     own MSE backward rounds d loss / d outputs differently from the fused loss kernel, so
    #     the comparison that can be exact feeds both paths the loss kernel's gradients)
    pc, ps = m2(*dbatch[:3])
    _, dc, dp = Trainer(m2, cfg).loss(pc.detach(), dbatch[3], ps.detach(), dbatch[1])
    torch.autograd.backward((pc, ps), (dc, dp))
    n_none = 0
    for n, p in m2.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, want[n]), n
        else:
            assert p.grad is None, n
            n_none += 1
    assert n_none == 142 - 55
    # (b) loss.backward() on torch's loss: the existing autograd test's gate, 1e-6 of max|g|
    opt.zero_grad()
    m2.load_state_dict(sd0)
    m2.train()
    m2.freeze("layer3")
    pc, ps = m2(*dbatch[:3])
    loss, _ = O.compute_loss(ocfg, pc, dbatch[3], ps, dbatch[1])
    loss.backward()
    for n, p in m2.named_parameters():
        if p.requires_grad:
            assert (p.grad - want[n]).abs().max() <= 1e-6 * max(1.0, float(want[n].abs().max())), n
        else:
            assert p.grad is None, n
    opt.step()
    sd = m2.state_dict()
    for n in _prefix_keys(sd0, 4):
        assert torch.equal(sd[n], sd0[n]), n
    assert not torch.equal(sd["visual_encoder.7.0.conv1.weight"], sd0["visual_encoder.7.0.conv1.weight"])
    # an image gradient through a frozen prefix is refused
    with pytest.raises(RuntimeError, match="input gradients"):
        m2(dbatch[0].clone().requires_grad_(), dbatch[1], dbatch[2])


# ---- 7. transitions -----------------------------------------------------------------------------------------
def test_freeze_two_steps_unfreeze_one_then_eval():
    from cilrs_mi355 import Trainer
    from cilrs_mi355.predict import Predictor
    cfg, ocfg = _cfgs()["A"]
    m, orc = _pair("A")
    tr = Trainer(m, cfg)
    opt = O.make_optimizer(orc, ocfg)            # ONE torch Adam lives through all three steps
    m.freeze("layer3")
    _idiom(orc, 4)
    for s in range(2):
        # later steps start from parameters that differ by Adam's lr * sign(g) ambiguity: losses
        # at 1e-3 there, as tests/test_model_gpu.py does; parameters within the hard bound
        _check_step(m, tr, orc, opt, cfg, ocfg, 4, True, seed=81 + s, outputs=(s == 0),
                    ltol=1e-4 if s == 0 else 1e-3, param_steps=s + 1)
    assert tr.group_steps == [0, 0, 0, 0, 2, 2]
    m.unfreeze()
    orc.train()
    for p in orc.parameters():
        p.requires_grad_(True)
    assert m.freeze_state() == (0, 0)
    _check_step(m, tr, orc, opt, cfg, ocfg, 0, True, seed=83, outputs=False, ltol=1e-3,
                param_steps=3)
    # the unfrozen tensors took their first update with step 1 (torch.optim.Adam's per-parameter
    # step), layer4 and the heads their third
    assert tr.group_steps == [1, 1, 1, 1, 3, 3]
    assert float(opt.state[next(orc.parameters())]["step"]) == 1.0
    # eval-mode inference sees the new weights: per-layer path and Predictor
    m.eval()
    orc.eval()
    imgs, spds, cmds = O.synthetic_batch(4, seed=84)[:3]
    with torch.no_grad():
        pc, ps = m(*to_dev(imgs, spds, cmds))
        opc, ops = orc(imgs, spds, cmds)
    assert float((pc.cpu() - opc).abs().max()) <= 1e-4 and float((ps.cpu() - ops).abs().max()) <= 1e-4
    pred = Predictor(m)
    frames = torch.randint(0, 256, (1, 88, 200, 3), dtype=torch.uint8,
                           generator=torch.Generator().manual_seed(85))
    got = pred.predict_controls(frames[0].numpy(), 12.0, 2)
    with torch.no_grad():
        want = O.predict_controls(orc, frames[0].numpy(), 12.0, 2)
    for a, b, tol in zip(got, want, (1e-4, 1e-4, 1e-4, 90 * 1e-4)):      # (speed in km/h: x 90)
        assert abs(float(a) - float(b)) <= tol, (got, want)


# ---- 8. refusals ----------------------------------------------------------------------------------------------
def _bad_patterns():
    def behind(m):
        m.visual_encoder[6].requires_grad_(False)
    def inside(m):
        m.freeze("stem")
        m.visual_encoder[4][1].conv2.weight.requires_grad_(False)
    def head(m):
        m.control_branches[1][3].weight.requires_grad_(False)
    def e_gt_g(m):
        m.freeze("stem")
        m.visual_encoder[4].eval()
    def bn_inside(m):
        m.visual_encoder[5][1].bn2.eval()
    return {"frozen group behind a trainable one": (behind, "visual_encoder.6.0.conv1.weight"),
            "one tensor frozen inside a group": (inside, "visual_encoder.4.1.conv2.weight"),
            "frozen head tensor": (head, "control_branches.1.3.weight"),
            "e > g": (e_gt_g, "visual_encoder.4.0.bn1"),
            "a BatchNorm in eval mode behind trainable groups": (bn_inside, "visual_encoder.5.1.bn2")}


@pytest.mark.parametrize("pattern", sorted(_bad_patterns()))
def test_unsupported_patterns_raise_before_any_launch(pattern):
    from cilrs_mi355 import Trainer
    apply, named = _bad_patterns()[pattern]
    cfg, _ = _cfgs()["A"]
    m, _ = _pair("A")
    tr = Trainer(m, cfg)
    dbatch = to_dev(*O.synthetic_batch(8, seed=91)[:4])
    apply(m)
    arena, bn, nbt = tr.eng.params.clone(), tr.eng.bn.clone(), tr.eng.nbt.clone()
    with pytest.raises(RuntimeError, match=named.replace(".", r"\.")):
        tr.train_step(*dbatch)
    with pytest.raises(RuntimeError, match=named.replace(".", r"\.")):
        m(*dbatch[:3])
    torch.cuda.synchronize()
    assert torch.equal(tr.eng.params, arena) and torch.equal(tr.eng.bn, bn)
    assert torch.equal(tr.eng.nbt, nbt) and tr.step_count == 0


def test_bf16_plan_and_fused_optimizer_refuse_a_freeze():
    from cilrs_mi355 import Trainer
    cfg, _ = _cfgs()["A"]
    dbatch = to_dev(*O.synthetic_batch(8, seed=92)[:4])
    m, _ = _pair("A")
    tr = Trainer(m, cfg, precision="bf16")
    m.freeze("layer1")
    arena = tr.eng.params.clone()
    with pytest.raises(RuntimeError, match="bf16"):
        tr.train_step(*dbatch)
    with pytest.raises(RuntimeError, match="bf16"):
        m(*dbatch[:3])
    assert torch.equal(tr.eng.params, arena)
    m, _ = _pair("A")
    tr = Trainer(m, cfg)
    tr.fuse_optimizer = True
    m.freeze("layer1")
    arena = tr.eng.params.clone()
    with pytest.raises(RuntimeError, match="fuse_optimizer"):
        tr.train_step(*dbatch)
    assert torch.equal(tr.eng.params, arena)
    # the C entries refuse a graph with a cut they cannot serve
    from cilrs_mi355 import _lib as L
    tr.fuse_optimizer = False
    tr.train_step(*dbatch)
    pl = tr.eng.last_plan
    dimage = torch.empty(8, 3, 88, 200, device="cuda")
    with pytest.raises(RuntimeError, match="froze"):
        tr.eng.run_input_grads(pl, dimage, None)
    with pytest.raises(RuntimeError, match="froze"):
        tr.eng.run_backward_step(pl, torch.zeros(8, 3, device="cuda"), torch.zeros(8, device="cuda"),
                                 tr.exp_avg, tr.exp_avg_sq, 1e-4, (0.9, 0.999), 1e-8, 0.0, 1)


# ---- 9. lr_mult ---------------------------------------------------------------------------------------------
def test_lr_mult_matches_torch_param_groups():
    from cilrs_mi355 import CONFIG_A, TrainConfig, Trainer
    from cilrs_mi355.train import GROUP_NAMES
    mult = {"stem": 0.01, "layer1": 0.05, "layer2": 0.1, "layer3": 0.3, "layer4": 0.5, "heads": 1.0}
    cfg = TrainConfig(**{**CONFIG_A.__dict__, "lr_mult": mult})
    ones = TrainConfig(**{**CONFIG_A.__dict__, "lr_mult": {n: 1.0 for n in GROUP_NAMES}})
    ms = [_pair("A")[0] for _ in range(3)]
    trs = [Trainer(ms[0], cfg), Trainer(ms[1], ones), Trainer(ms[2], CONFIG_A)]
    eng = trs[0].eng
    # torch: one param group per trunk group and heads, on CPU copies of the same parameters
    ref = [p.detach().cpu().clone().requires_grad_(True) for p in ms[0].parameters()]
    groups = [[] for _ in range(6)]
    for t, (_, off, _, _) in zip(ref, eng.params_layout):
        gi = next(i for i, (b, e) in enumerate(eng.group_ranges) if b <= off < e)
        groups[gi].append(t)
    opt = torch.optim.Adam([dict(params=ps, lr=CONFIG_A.lr * mult[n])
                            for ps, n in zip(groups, GROUP_NAMES)], lr=CONFIG_A.lr,
                           betas=CONFIG_A.betas, eps=CONFIG_A.eps, weight_decay=CONFIG_A.weight_decay)
    g = torch.Generator().manual_seed(11)
    for step in range(3):
        if step == 2:
            for tr in trs:
                tr.scheduler_step()                       # scales every group
                tr.lr = tr.lr * 0.5                       # (StepLR steps at epoch 8: force a change)
            for pg in opt.param_groups:
                pg["lr"] *= 0.5
        for t, gv0, gv1, gv2 in zip(ref, *(tr.eng.grad_views for tr in trs)):
            gr = torch.randn(t.shape, generator=g) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=g))
            t.grad = gr.clone()
            for gv in (gv0, gv1, gv2):
                gv.copy_(gr)
        opt.step()
        for tr in trs:
            tr.optimizer_step()
    torch.cuda.synchronize()
    worst = 0.0
    for t, p in zip(ref, ms[0].parameters()):
        worst = max(worst, float((p.detach().cpu() - t.detach()).abs().max()))
    print(f"lr_mult: worst element after three steps {worst:.2e}")
    assert worst <= 1e-6
    assert torch.equal(trs[1].eng.params, trs[2].eng.params)
    assert torch.equal(trs[1].exp_avg, trs[2].exp_avg) and torch.equal(trs[1].exp_avg_sq, trs[2].exp_avg_sq)
    assert not torch.equal(trs[0].eng.params, trs[2].eng.params)


# ---- 10. checkpoint ---------------------------------------------------------------------------------------------
def test_checkpoint_resumes_a_fine_tuning_run_bit_identically(tmp_path):
    """Config A: no dropout, so the resumed run needs no dropout-seed state (the Trainer's dropout
    call counter is not part of the reference's checkpoint layout)."""
    from cilrs_mi355 import Trainer, checkpoint
    cfg, _ = _cfgs()["A"]
    batches = [to_dev(*O.synthetic_batch(8, seed=101 + s)[:4]) for s in range(3)]
    m, _ = _pair("A")
    m.freeze("layer2")
    tr = Trainer(m, cfg)
    for s in range(2):
        tr.train_step(*batches[s])
    path = os.path.join(str(tmp_path), "latest.pth")
    checkpoint.save_latest(path, m, tr, epoch=0)
    ck = checkpoint.load_file(path)
    st = ck["optimizer_state_dict"]["state"]
    assert len(st) == 142
    assert float(st[0]["step"]) == 0.0 and float(st[141]["step"]) == 2.0
    assert not st[0]["exp_avg"].any() and st[141]["exp_avg"].any()
    tr.train_step(*batches[2])
    torch.cuda.synchronize()
    m2, _ = _pair("A")
    m2.freeze("layer2")
    tr2 = Trainer(m2, cfg)
    checkpoint.load(path, m2, tr2)
    m2.train()
    m2.freeze("layer2")                  # load() does not change flags; train() cleared the eval ones
    assert tr2.group_steps == [0, 0, 0, 2, 2, 2]
    tr2.train_step(*batches[2])
    torch.cuda.synchronize()
    assert torch.equal(tr.eng.params, tr2.eng.params)
    assert torch.equal(tr.eng.bn, tr2.eng.bn) and torch.equal(tr.eng.nbt, tr2.eng.nbt)
    assert torch.equal(tr.exp_avg, tr2.exp_avg) and torch.equal(tr.exp_avg_sq, tr2.exp_avg_sq)
    assert torch.equal(tr.loss_buf[:6], tr2.loss_buf[:6])


# ---- 11. two ranks on one GPU --------------------------------------------------------------------------------
def _dp_worker(rank, world, port, q, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from cilrs_mi355 import CILRS, CONFIG_A, Trainer
        from cilrs_mi355.parallel import broadcast_parameters
        torch.cuda.set_device(0)
        m = CILRS(4, dropout=0.0)
        m.load_state_dict(_warm_state("A"), strict=True)
        m = m.cuda().train()
        m.freeze("layer2")
        tr = Trainer(m, CONFIG_A, process_group=dist.group.WORLD)
        broadcast_parameters(tr.eng, dist.group.WORLD)
        sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        imgs, spds, cmds, tgts = O.synthetic_batch(4, seed=160 + rank)[:4]
        tr.train_step(imgs.cuda(), spds.cuda(), cmds.cuda(), tgts.cuda())
        loss = tr.losses()["total"]
        cut = tr.eng.trainable_begin(3)
        extra = {"grads": {n: (g.detach().cpu() * tr.arena_grad_scale).contiguous()
                           for (n, off, _, _), g in zip(tr.eng.params_layout, tr.eng.grad_views)
                           if off >= cut},
                 "collectives": tr.reducer.collectives, "sd0": sd0}
        torch.cuda.synchronize()
        torch.save({k: v.detach().cpu() for k, v in m.state_dict().items()},
                   os.path.join(out_dir, f"rank{rank}.pt"))
        torch.save(extra, os.path.join(out_dir, f"rank{rank}_extra.pt"))
        q.put((rank, None, loss))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:                                   # surface the failure in the parent
        import traceback
        q.put((rank, traceback.format_exc() + str(e), None))


def test_two_ranks_reduce_only_the_trainable_ranges(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(120)
    for r in res:
        assert r[1] is None, r[1]
    sds = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt"), weights_only=True) for r in range(2)]
    ex = [torch.load(os.path.join(str(tmp_path), f"rank{r}_extra.pt"), weights_only=True)
          for r in range(2)]
    frozen = set(_prefix_keys(sds[0], 3))
    for k in sds[0]:
        if k in frozen:
            assert torch.equal(sds[0][k], ex[0]["sd0"][k]) and torch.equal(sds[1][k], ex[1]["sd0"][k]), k
        if "running_" in k or "num_batches" in k:
            continue
        assert torch.equal(sds[0][k], sds[1][k]), k                 # replicas bit-identical
    # buckets: layer4 + heads, layer3; stem + layer1 + layer2 lies wholly inside the prefix
    assert ex[0]["collectives"] == 2 and ex[1]["collectives"] == 2
    # oracle: the two shards' gradients averaged, on the trainable tensors
    grads = []
    for rank in range(2):
        orc = O.build_oracle(0)
        orc.load_state_dict(_warm_state("A"), strict=True)
        orc.train()
        _idiom(orc, 3)
        imgs, spds, cmds, tgts = O.synthetic_batch(4, seed=160 + rank)[:4]
        pc, ps = orc(imgs, spds, cmds)
        loss, _ = O.compute_loss(O.CONFIG_A, pc, tgts, ps, spds)
        loss.backward()
        assert abs(res[rank][2] - float(loss.detach())) <= 1e-4 * max(1.0, float(loss.detach()))
        grads.append({n: p.grad for n, p in orc.named_parameters()})
    n_live = 0
    for n, a in grads[0].items():
        if a is None:
            assert n not in ex[0]["grads"]
            continue
        n_live += 1
        want = (a + grads[1][n]) / 2
        nrm = max(float(want.norm()), 1e-12)
        for r in range(2):
            assert float((ex[r]["grads"][n] - want).norm()) <= 1e-2 * nrm, (n, r)
        assert torch.equal(ex[0]["grads"][n], ex[1]["grads"][n]), n
    assert n_live == 94 == len(ex[0]["grads"])


# ---- 12. the ResNet-50 variant ----------------------------------------------------------------------------------
def test_resnet50_variant_frozen_prefix_step():
    from cilrs_mi355 import Trainer
    cfg, ocfg = _cfgs()["B"]
    m, orc = _pair("B", variant=1, batch=4)
    m.freeze("layer2")
    _idiom(orc, 3)
    assert m.freeze_state() == (3, 3)
    tr = Trainer(m, cfg)
    opt = O.make_optimizer(orc, ocfg)
    _check_step(m, tr, orc, opt, cfg, ocfg, 3, True, seed=121, batch_size=4)
