"""Host checks of tests/_eval32_walk.py, the layer-by-layer walk of the fp32 eval forward: driven by
a CPU backend (every tensor computed step by step in torch fp32) it passes at the shapes the GPU
tests use, its wiring -- fold, flags, residual order -- reproduces the oracle's own visual encoder,
and sabotaged backends each make it fail at exactly the sabotaged tensor.

What each sabotage does to the four network outputs (perturbed-statistics weights, synthetic frame
of seed 123; max |sabotaged - clean| over steer, throttle, brake, raw speed and the four commands),
beside the walk's worst error-to-bound ratio on the sabotaged tensor:
                                                              (1, 88, 200)          (1, 30, 70)
  corner tap (2,2) dropped at pixel (0,0) of block 3 conv1    1.1e-3   10,688 x     9.7e-3   14,048 x
  ... for input channel 0 of its 64 alone                     1.3e-4    1,032 x     6.4e-4    1,613 x
  ReLU before the residual in block 9 (layer3.2)              9.7e-2    9,559 x     8.2e-2    7,215 x
  last pixel of block 7 conv2 (M = 78 / 10) left stale        3.7e-3   15,159 x     1.6e-2    9,868 x
With these weights and this frame every one of them also moves the outputs by more than the 1e-4
of the output-level test (which runs other weights at 88x200 only): by a factor of 1.3 for the
one-channel tap, 11 to 970 for the others.  The walk sees them by a factor of 1,000 to 15,000 on
the one tensor they sit on, and names it.
"""
import pytest
import torch

import cilrs_oracle as O
import infer16_emulation as E
import _eval32_walk as K

SHAPES = [(1, 88, 200), (1, 30, 70)]
_CACHE = {}


def _oracle():
    if "orc" not in _CACHE:
        orc = O.build_oracle(0)
        orc.load_state_dict(E.perturbed_state_dict(O.portable_state_dict(orc.state_dict(), 0), 0))
        _CACHE["orc"] = orc.eval()
    return _CACHE["orc"]


def _clean(shape, seed=123):
    """(inputs, clean CPU backend) of a shape, computed once."""
    key = (shape, seed)
    if key not in _CACHE:
        B, H, W = shape
        img, spd, cmd = O.synthetic_batch(B, seed=seed, h=H, w=W)[:3]
        _CACHE[key] = ((img, spd, cmd), K.CpuBackend(_oracle(), img, spd, cmd))
    return _CACHE[key]


@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_backend_passes_the_walk_and_is_the_oracles_encoder(shape):
    orc = _oracle()
    (img, spd, cmd), be = _clean(shape)
    rows, last = K.walk(orc, be.x4, be.fetch, cmd, spd, be.outputs, image=img, R=2, what=f"cpu {shape}")
    assert len(rows) == 36 and sorted(r["conv"] for r in rows) == list(range(36))
    assert max(r["bound_ratio"] for r in rows) <= 0.1       # torch's fp32: far inside the contract
    with torch.no_grad():
        want = orc.visual_encoder(img)
        oc, os_ = orc(img, spd, cmd)
    got = E.avgpool(last, torch.float32)
    err = float((got - want).abs().max())
    print(f"EVAL32 cpu {shape}: walked feature vector vs orc.visual_encoder {err:.3e}")
    assert err <= 1e-5
    assert float((be.outputs[0] - oc).abs().max()) <= 1e-5 and float((be.outputs[1] - os_).abs().max()) <= 1e-5


def _ragged_step(orc, shape):
    """A step of the walk whose output pixel count is no multiple of 16 (a ragged last tile)."""
    (img, spd, cmd), be = _clean(shape)
    for name in ("block 7 conv2", "block 13 conv2", "block 3 conv2"):
        t = be.by_name[name]
        if (t.shape[0] * t.shape[2] * t.shape[3]) % 16:
            return name
    raise AssertionError("no ragged tensor at this shape")


@pytest.mark.parametrize("kind", ["tap", "tap1", "relu", "stale"])
@pytest.mark.parametrize("shape", SHAPES)
def test_walk_fails_at_exactly_the_sabotaged_tensor(shape, kind):
    orc = _oracle()
    (img, spd, cmd), clean = _clean(shape)
    where = {"tap": "block 3 conv1", "tap1": "block 3 conv1", "relu": "block 9 conv2"}.get(kind) or \
        _ragged_step(orc, shape)
    previous = _clean(shape, seed=7)[1] if kind == "stale" else None
    bad = K.CpuBackend(orc, img, spd, cmd, (kind, where), previous)
    assert not torch.equal(bad.by_name[where], clean.by_name[where])
    with pytest.raises(K.WalkFailure) as info:
        K.walk(orc, bad.x4, bad.fetch, cmd, spd, bad.outputs, image=img, R=2, what=f"{kind} {shape}")
    print(f"EVAL32 sabotage {kind} at {where} {shape}: {info.value}")
    assert info.value.tensors() == [where]
    # what the output-level tests could see of it: the four outputs, every command
    moved = 0.0
    for c in range(4):
        cc = torch.full_like(cmd, c)
        a = torch.cat([t.view(len(cc), -1) for t in E.heads(orc, E.avgpool(bad.last, torch.float32), spd, cc)], 1)
        b = torch.cat([t.view(len(cc), -1) for t in E.heads(orc, E.avgpool(clean.last, torch.float32), spd, cc)], 1)
        moved = max(moved, float((a - b).abs().max()))
    print(f"EVAL32 sabotage {kind} at {where} {shape}: the four outputs move by at most {moved:.3e}")


def test_walk_reports_wrong_heads_and_a_wrong_pool():
    """The two checks that are not convolution steps fail under their own names."""
    orc = _oracle()
    (img, spd, cmd), be = _clean((1, 30, 70))
    off = (be.outputs[0] + 1e-3, be.outputs[1])
    with pytest.raises(K.WalkFailure) as info:
        K.walk(orc, be.x4, be.fetch, cmd, spd, off, image=img, R=2)
    assert info.value.tensors() == ["heads"]
    pool = be.z[-1].clone()
    pool[0, 3, 0, 0] = be.z[0][0, 3, 2, 2]              # a window one pixel off
    assert not torch.equal(pool, be.z[-1])
    with pytest.raises(K.WalkFailure) as info:
        K.walk(orc, be.x4, lambda i: pool if i == -1 else be.z[i], cmd, spd, be.outputs, image=img, R=2)
    assert "max-pool" in info.value.tensors()
