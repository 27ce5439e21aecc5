"""The fp32 eval-mode forward, layer by layer, in both of its realisations: the per-layer launches
(trunk_fwd_eval32: conv_small.hip or the implicit-GEMM kernel with the folded BatchNorm / ReLU /
residual epilogue) and the persistent single-frame launch (csrc/infer_b1.hip).  Both leave every
stage's output in the plan's workspace; tests/_eval32_walk.py compares each of them with a float64
computation on the tensor the SAME realisation stored one step earlier (its docstring has the
reference, the flags and the four assertions per tensor).

Measured on an MI355X (256 workgroups), all cases of this file, 36 convolution tensors each:
  largest e_hip / e_cpu  1.713  per-layer (17,40,120) block 7 downsample (conv 18, 1x1 stride 2,
                         implicit GEMM); the persistent launch's largest is 0.952 (88x200, conv 18);
                         hence R_NOISE = ceil(2 x 1.713) = 4
  worst error / bound    0.0217 per-layer (3,88,200) stem; persistent launch 0.0124; heads <= 0.017
  max-pool bit-equal and x4 equal to the oracle's normalised image (0.0) in every case.

Which kernel served the per-layer cases: BY THE ROUTING RULE of trunk_fwd_eval32 and the constants
kSmallConvBlocks = 256, kSmallConvK = 2304 (restated in _routing; both kernels run under the same
profile label and no accessor tells them apart, so this is not observed on the device):
  (1,88,200)   layer1 implicit GEMM (276 tiles); layer2 (144), layer3 (80), layer4.0.conv1 and
               layer4's downsample (64) conv_small; layer4's other 3x3 (K = 4608) implicit GEMM
  (1,30,70)    everything on conv_small (36, 24, 16, 32 tiles) but layer4's K = 4608 convolutions
  (3,88,200)   layer1 (828), layer2 (416) implicit GEMM; layer3 (240) conv_small; layer4 as above
  (17,40,120)  everything on implicit GEMM (1276, 640, 416, 288 tiles)
  (1,176,400)  (after the planner's refusal) layer1-3 implicit GEMM, layer4 as at (1,88,200)

Tilings of the persistent launch as cilrs_net_b1_stage_info reported them (wpt of the stem; every
other convolution stage has wpt 16; "pair" = the two-convolution stage of a layer's first block,
conv1 | downsample; same_shape is 1 on every stage that follows a one-convolution stage of its
own shape, i.e. all but the first two stages of a layer):
  geometry  stem wpt  layer1        layer2                layer3               layer4
  88x200    2         ks 1 nt 2     pair nt 1 | nt 2,     pair ks 2 | 1,       pair ks 3 | 1,
                                    then ks 1 nt 1        then ks 3            then ks 4
  96x160    4         ks 1 nt 1     pair ks 1, then ks 2  pair ks 3 | 1, ks 4  pair ks 4 | 1, ks 4
  40x120    8         ks 1 nt 1     pair ks 1, then ks 4  pair ks 4 | 1, ks 4  pair ks 4 | 1, ks 4
  64x64     16        ks 1 nt 1     pair ks 1, then ks 4  pair ks 4 | 1, ks 4  pair ks 4 | 1, ks 4
  30x70     16        ks 1 nt 1     (as 64x64)
Together: wpt {2, 4, 8, 16}, ksplit {1, 2, 3, 4}, nt {1, 2}, a two-convolution stage with nt = 2
(88x200, layer2), same_shape {0, 1} -- asserted by test_persistent_geometries_cover_the_planner.
176x400 is refused ("no one-pass tiling of a stage on 256 workgroups") before anything is launched.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import cilrs_oracle as O
import _eval32_walk as K

pytestmark = pytest.mark.gpu

# Noise gate: e_hip <= R * max(e_cpu, 1e-7 * rms(ref)), e_cpu from torch's fp32 CPU realisation of the
# same step.  R = twice the largest ratio measured over every case of this file, rounded up, at
# least 2 (see the docstring for the ratio and its tensor).
R_NOISE = 4

_STAGES = 3 + 2 * 16 + 3
_SEEN = {"ratio": (0.0, ""), "bound": (0.0, ""), "tilings": {}}
_CACHE = {}


def _lib():
    from cilrs_mi355 import _lib as L
    return L


def _pair():
    """(engine-backed module on the GPU, CPU oracle) with the perturbed-statistics weights, once."""
    if "pair" not in _CACHE:
        _CACHE["pair"] = K._models("resnet34")
    return _CACHE["pair"]


def _inputs(B, H, W, seed=123):
    img, spd, cmd, _, u8 = O.synthetic_batch(B, seed=seed, h=H, w=W)
    return img, spd, cmd, torch.from_numpy(u8)


class _PlanView:
    """What a plan's fp32 eval forward left in the workspace, through the accessors."""

    def __init__(self, pl):
        self.pl, self.L = pl, _lib()

    def fetch(self, conv):
        """Stored output of convolution `conv` (-1: the max-pool), [B][C][H*W] on the CPU."""
        L, pl = self.L, self.pl
        yo, zo, n, ch = L.sz(), L.sz(), L.sz(), L.i32()
        L.check(L.lib().cilrs_net_activation_info(pl.handle, conv, C.byref(yo), C.byref(zo),
                                                  C.byref(n), C.byref(ch)))
        z = pl.workspace.view(torch.float32)[zo.value:zo.value + n.value]
        return z.view(pl.batch, -1, ch.value).permute(0, 2, 1).contiguous().cpu()

    def x4(self):
        L, pl = self.L, self.pl
        xo, xn = L.sz(), L.sz()
        L.check(L.lib().cilrs_net_infer16_io_info(pl.handle, C.byref(xo), C.byref(xn), None, None, None))
        x = pl.workspace[xo.value:xo.value + 4 * xn.value].view(torch.float32).cpu()
        return x.view(pl.batch, pl.h, pl.w, 4)

    def stages(self):
        """[dict(type, wpt, same_shape, workgroups, convs=[(number, ksplit, nt)])] of the persistent
        launch's stage table (cilrs_net_b1_stage_info)."""
        L, pl = self.L, self.pl
        out = []
        for s in range(L.lib().cilrs_net_b1_stages(pl.handle)):
            ty, wpt, same, wg, nc = L.i32(), L.i32(), L.i32(), L.i32(), L.i32()
            conv, ks, nt = (L.i32 * 2)(), (L.i32 * 2)(), (L.i32 * 2)()
            L.check(L.lib().cilrs_net_b1_stage_info(pl.handle, s, C.byref(ty), C.byref(wpt),
                                                    C.byref(same), C.byref(wg), C.byref(nc), conv, ks, nt))
            out.append(dict(type=ty.value, wpt=wpt.value, same_shape=same.value, workgroups=wg.value,
                            convs=[(conv[i], ks[i], nt[i]) for i in range(nc.value)]))
        return out


def _note(rows, what):
    for r in rows:
        if r["ratio"] > _SEEN["ratio"][0]:
            _SEEN["ratio"] = (r["ratio"], f"{what} {r['name']} (conv {r['conv']})")
        if r["bound_ratio"] > _SEEN["bound"][0]:
            _SEEN["bound"] = (r["bound_ratio"], f"{what} {r['name']} (conv {r['conv']})")


# ---- per-layer launches ----------------------------------------------------------------------------
def _routing(orc, B, H, W):
    """Which kernel trunk_fwd_eval32 picks for every trunk convolution, restated from its rule and
    the constants of csrc/common.h (kSmallConvBlocks = 256 tiles of 16 x 16, kSmallConvK = 2304):
    conv_small unless ceil(M / 16) * (Cout / 16) > 256 or K * K * Cin > 2304.  {layer: set of
    kernels}, layer = 1..4 (ResNet layer of the convolution).  Neither the profile labels (both
    kernels run under "conv_fwd.<group>") nor an accessor tell the two apart on the device, so
    this is a statement about the rule, not an observation."""
    out = {}
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for bi, blk in enumerate(K.E.trunk_blocks(orc)):
        layer = 1 + sum(bi >= n for n in (3, 7, 13))
        main, down = K.E.block_convs(blk)
        s = main[0][0].stride[0]
        h, w = (h - 1) // s + 1, (w - 1) // s + 1
        M = B * h * w
        for conv, _bn in main + ([down] if down else []):
            k = conv.kernel_size[0]
            tiles = -(-M // 16) * (conv.out_channels // 16)
            small = tiles <= 256 and k * k * conv.in_channels <= 2304
            out.setdefault(layer, set()).add("small" if small else "igemm")
            out.setdefault((layer, "tiles"), set()).add(tiles)
    return out


# (B, H, W) -> the kernels each ResNet layer takes by the constants
PER_LAYER_CASES = {
    # the control loop's shape: layer1 276 tiles -> implicit GEMM (tile epilogue); layer2, layer3,
    # layer4.0.conv1 and the downsamples -> conv_small; layer4's 3x3 with K = 4608 -> implicit GEMM
    # (few tiles, long reduction: split-K and its reduce epilogue)
    (1, 88, 200): {1: {"igemm"}, 2: {"small"}, 3: {"small"}, 4: {"small", "igemm"}},
    # odd sizes at every level (15x35, 8x18, 4x9, 2x5, 1x3): layer4 M = 3 < one tile, layer3 M = 10;
    # layer1 on conv_small too
    (1, 30, 70): {1: {"small"}, 2: {"small"}, 3: {"small"}, 4: {"small", "igemm"}},
    # layer2 moves to implicit GEMM (416 tiles); layer3 stays on conv_small with 240 of 256 tiles
    (3, 88, 200): {1: {"igemm"}, 2: {"igemm"}, 3: {"small"}, 4: {"small", "igemm"}},
    # every convolution on implicit GEMM: layer4.0.conv1 and its downsample have M = 136 -> 9 x 32 =
    # 288 tiles (B = 16: exactly 256, still conv_small); M = 5100, 1275, 408, 136 (20x60 after the
    # stem, 10x30, 5x15, 3x8, 2x4 per frame): ragged last tiles in layer1, layer2, layer3 and layer4
    (17, 40, 120): {1: {"igemm"}, 2: {"igemm"}, 3: {"igemm"}, 4: {"igemm"}},
}


def _walk_per_layer(B, H, W):
    m, orc = _pair()
    eng = m.engine()
    img, spd, cmd, u8 = _inputs(B, H, W)
    c, s = eng.run_forward_u8(u8.cuda(), spd.cuda(), cmd.cuda(), graph=False, half=False,
                              persistent=False)
    torch.cuda.synchronize()
    eng.check_status()
    view = _PlanView(eng.last_plan)
    what = f"per-layer ({B},{H},{W})"
    rows, _last = K.walk(orc, view.x4(), view.fetch, cmd, spd, (c.cpu(), s.cpu()), image=img,
                         R=R_NOISE, what=what)
    assert len(rows) == 36
    _note(rows, what)
    return rows


@pytest.mark.parametrize("B,H,W", list(PER_LAYER_CASES))
def test_per_layer_launches_layer_by_layer(B, H, W):
    _m, orc = _pair()
    route = _routing(orc, B, H, W)
    print(f"EVAL32 per-layer ({B},{H},{W}) routing by the constants:",
          {k: sorted(v) for k, v in route.items()})
    assert {k: v for k, v in route.items() if isinstance(k, int)} == PER_LAYER_CASES[(B, H, W)]
    if (B, H, W) == (3, 88, 200):
        assert 240 in route[(3, "tiles")]                 # just under the 256-tile threshold
    if (B, H, W) == (17, 40, 120):
        assert 288 in route[(4, "tiles")]                 # just over it (B = 16: exactly 256)
    _walk_per_layer(B, H, W)


# ---- the persistent launch ---------------------------------------------------------------------------
PERSISTENT_GEOMETRIES = [(88, 200), (96, 160), (40, 120), (64, 64), (30, 70)]


def _table_text(stages):
    lines = []
    for i, st in enumerate(stages):
        if st["convs"]:
            cv = " | ".join(f"conv {n} ks {ks} nt {nt}" for n, ks, nt in st["convs"])
            lines.append(f"stage {i} wpt {st['wpt']} same {st['same_shape']}: {cv}")
    return "; ".join(lines)


@pytest.mark.parametrize("H,W", PERSISTENT_GEOMETRIES)
def test_persistent_launch_layer_by_layer(H, W):
    """One trunk walk per geometry on the launch for command 0, then one launch per further
    command with the heads check on the feature map that launch stored."""
    m, orc = _pair()
    eng = m.engine()
    img, spd, _cmd, u8 = _inputs(1, H, W)
    frames, spd_d = u8.cuda(), spd.cuda()
    what = f"persistent {H}x{W}"
    last_conv = last_shape = None
    for c in range(4):
        cmd = torch.tensor([c], dtype=torch.int64)
        ctrl, ps = eng.run_forward_u8(frames, spd_d, cmd.cuda(), persistent=True)
        torch.cuda.synchronize()
        out = (ctrl.cpu(), ps.cpu())
        view = _PlanView(eng.last_plan)
        if c == 0:
            rows, last = K.walk(orc, view.x4(), view.fetch, cmd, spd, out, image=img, R=R_NOISE,
                                what=what)
            assert len(rows) == 36
            _note(rows, what)
            last_conv, last_shape = rows[-1]["conv"], last.shape
        else:
            K.check_heads(orc, view.fetch(last_conv).view(last_shape), spd, cmd, out, what)
    pl = eng.last_plan
    assert _lib().lib().cilrs_net_b1_stages(pl.handle) == _STAGES
    eng.check_status()                                     # no barrier gave up, no bad command
    stages = _PlanView(pl).stages()
    assert len(stages) == _STAGES
    assert [st["type"] for st in stages] == [0, 2, 3] + [1] * 32 + [4] * 3
    numbered = sorted(n for st in stages for n, _ks, _nt in st["convs"])
    assert numbered == list(range(36))                     # every convolution in exactly one stage
    print(f"EVAL32 {what} tiling on {stages[0]['workgroups']} workgroups: {_table_text(stages)}")
    _SEEN["tilings"][(H, W)] = stages


def test_persistent_geometries_cover_the_planner():
    """Runs after the five geometries: together they must have taken every branch of b1_build
    (on the 256-workgroup grid the cases were chosen for; on another grid the table is printed)."""
    tl = _SEEN["tilings"]
    assert sorted(tl) == sorted(PERSISTENT_GEOMETRIES), "run the whole file: this test sums up the walks"
    conv_stages = [st for stages in tl.values() for st in stages if st["convs"]]
    wpt = {st["wpt"] for st in conv_stages}
    ks = {k for st in conv_stages for _n, k, _t in st["convs"]}
    nt = {t for st in conv_stages for _n, _k, t in st["convs"]}
    pair_nt2 = any(len(st["convs"]) == 2 and any(t == 2 for _n, _k, t in st["convs"]) for st in conv_stages)
    same = {st["same_shape"] for st in conv_stages}
    stem = {hw: stages[1]["wpt"] for hw, stages in tl.items()}
    print(f"EVAL32 persistent coverage: wpt {sorted(wpt)} ksplit {sorted(ks)} nt {sorted(nt)} "
          f"two-convolution stage with nt=2 {pair_nt2} same_shape {sorted(same)} stem wpt {stem}")
    grids = {stages[0]["workgroups"] for stages in tl.values()}
    if grids != {256}:
        print(f"EVAL32 persistent coverage: grid {sorted(grids)} is not 256 workgroups, nothing asserted")
        return
    assert wpt == {2, 4, 8, 16} and ks == {1, 2, 3, 4} and nt == {1, 2} and pair_nt2 and same == {0, 1}


# ---- a geometry the planner refuses --------------------------------------------------------------------
def test_planner_refusal_then_per_layer_and_predictor_fallback():
    """176x400: 88 x 200 = 17,600 stem pixels = 1,100 row tiles x 4 channel tiles = 4,400 units
    against 256 workgroups x 8 two-wave groups = 2,048 slots -> b1_build has no one-pass tiling.
    The refusal comes before anything is launched and leaves the status words clean; the per-layer
    path on the same engine then serves the frame and passes its walk; a Predictor of that size
    (persistent by default at batch 1) answers with the per-layer path's numbers."""
    from cilrs_mi355.predict import Predictor
    m, orc = _pair()
    eng = m.engine()
    H, W = 176, 400
    img, spd, cmd, u8 = _inputs(1, H, W)
    ctrl = torch.full((1, 3), 7.0, device="cuda")
    ps = torch.full((1,), 7.0, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="tiling"):
        eng.run_forward_u8(u8.cuda(), spd.cuda(), cmd.cuda(), out=(ctrl, ps), persistent=True)
    torch.cuda.synchronize()
    pl = eng.plan(1, H, W)
    assert _lib().lib().cilrs_net_b1_stages(pl.handle) == -1            # never launched
    assert pl.status.tolist() == [0, 0, 0, 0]
    assert (ctrl == 7.0).all() and (ps == 7.0).all()                    # nothing wrote the outputs
    pl.check_status()
    _walk_per_layer(1, H, W)
    # the control-loop adapter
    frame = u8[0].numpy()
    kmh, c = 37.0, 2
    eager = Predictor(m, height=H, width=W, persistent=False)
    want = eager.predict_controls(frame, kmh, c)
    pred = Predictor(m, height=H, width=W)
    assert pred.persistent                                              # the default at batch 1
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        got = pred.predict_controls(frame, kmh, c)
        again = pred.predict_controls(frame, kmh, c)
    assert not pred.persistent
    assert got == want == again, (got, want, again)
    assert sum("tiling" in str(w.message) for w in wlist) == 1
    assert np.isfinite(got).all()
    pred.eng.check_status()
    # a raw camera frame of another size: the fused resize in front of the same fallback
    cam = np.ascontiguousarray(np.resize(frame, (300, 500, 4)))
    want_cam = eager.predict_camera(cam, kmh, c)
    pred2 = Predictor(m, height=H, width=W)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        got_cam = pred2.predict_camera(cam, kmh, c)
    assert not pred2.persistent and got_cam == want_cam, (got_cam, want_cam)
    assert sum("tiling" in str(w.message) for w in wlist) == 1
    pred2.eng.check_status()


def test_eval32_report():
    """Runs last in this file: the figures the module docstring records."""
    print(f"EVAL32 largest e_hip/e_cpu {_SEEN['ratio'][0]:.3f} at {_SEEN['ratio'][1]}; worst "
          f"error-to-bound ratio {_SEEN['bound'][0]:.4f} at {_SEEN['bound'][1]}; R_NOISE {R_NOISE}")
