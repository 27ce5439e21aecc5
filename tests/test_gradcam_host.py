"""The float64 statement of Grad-CAM (tests/_gradcam.py) against torch.autograd on the oracle
network, its upsample against F.interpolate, and the argument checks of Predictor.gradcam that need
no device."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gradcam as GC
import cilrs_oracle as O

FRAMES = {"88x200": (88, 200, 21), "40x72": (40, 72, 22)}
WEIGHTS = (0.75, -0.5, 0.25, 1.5)
_CACHE = {}


def _oracle64():
    if "orc" not in _CACHE:
        _CACHE["orc"] = O.build_oracle(0).double().eval()
    return _CACHE["orc"]


def _autograd(frame, layer):
    key = (frame, layer)
    if key not in _CACHE:
        h, w, seed = FRAMES[frame]
        img, spd, cmd, _t, _u8 = O.synthetic_batch(1, seed=seed, h=h, w=w)
        _CACHE[key] = (img, spd, cmd) + GC.autograd_gradcam(_oracle64(), img.double(), spd.double(),
                                                            cmd, WEIGHTS, layer)
    return _CACHE[key]


@pytest.mark.parametrize("frame", list(FRAMES))
def test_layer4_closed_form_equals_autograd(frame):
    _img, spd, cmd, A, dA, cam, out = _autograd(frame, 4)
    B, h, w, C = A.shape
    assert (h, w, C) == ((3, 7, 512) if frame == "88x200" else (2, 3, 512))
    r = GC.heads_input_grad64(_oracle64(), A.mean(dim=(1, 2)), spd, cmd, WEIGHTS)
    # avgpool sits on layer4: dA is g / (h*w) in every cell
    want = (r["g"] / (h * w))[:, None, None, :].expand(B, h, w, C)
    scale = float(dA.abs().max())
    assert scale > 0.0
    assert float((dA - want).abs().max()) <= 1e-12 * scale
    assert float((out - r["out"]).abs().max()) <= 1e-12 * max(1.0, float(out.abs().max()))
    d = GC.gradcam64(A.numpy(), h * 8, w * 8, g=r["g"].numpy())
    assert float(np.abs(d["cam"] - cam.numpy()).max()) <= 1e-12 * float(cam.abs().max())
    assert np.abs(d["alpha"] - dA.mean(dim=(1, 2)).numpy()).max() <= 1e-12 * scale
    # the error scale of g dominates g itself
    assert bool((r["S"] >= r["g"].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("frame", list(FRAMES))
def test_layer3_definition_equals_autograd(frame):
    _img, _spd, _cmd, A, dA, cam, _out = _autograd(frame, 3)
    B, h, w, C = A.shape
    assert (h, w, C) == ((6, 13, 256) if frame == "88x200" else (3, 5, 256))
    d = GC.gradcam64(A.numpy(), 88, 200, dA=dA.numpy())
    assert float(np.abs(d["cam"] - cam.numpy()).max()) <= 1e-12 * float(cam.abs().max())
    assert float(cam.abs().max()) > 0.0
    # deeper than layer4 the gradient is no longer constant over the cells
    assert float(dA.std(dim=(1, 2)).max()) > 0.0
    n, peak = GC.normalise64(cam.numpy())
    assert n.min() >= 0.0 and (n.max() == 1.0 or peak[0] == 0.0)
    assert d["heat"].shape == (B, 88, 200) and d["heat"].min() >= 0.0 and d["heat"].max() <= 1.0
    assert bool((d["cam_scale"] >= np.abs(d["cam"]) * (1 - 1e-12)).all())


@pytest.mark.parametrize("shape,size", [((2, 3, 7), (88, 200)), ((1, 1, 1), (8, 8)),
                                        ((3, 2, 5), (33, 47)), ((1, 22, 50), (88, 200)),
                                        ((1, 6, 13), (88, 200)), ((1, 5, 4), (5, 4))])
def test_upsample_equals_interpolate(shape, size):
    n = torch.from_numpy(O._hash_u01(7, 3000, int(np.prod(shape))).astype(np.float64)).view(shape)
    want = F.interpolate(n.unsqueeze(1), size=size, mode="bilinear", align_corners=False).squeeze(1)
    got = GC.upsample64(n.numpy(), *size)
    assert np.abs(got - want.numpy()).max() <= 1e-14
    if shape[1:] == (1, 1):
        assert np.array_equal(got, np.full_like(got, float(n.view(-1)[0])))
    if tuple(shape[1:]) == tuple(size):
        assert np.array_equal(got, n.numpy())


def test_all_negative_map_normalises_to_zero():
    cam = -np.abs(O._hash_u01(3, 3001, 21).astype(np.float64)).reshape(1, 3, 7) - 0.1
    n, peak = GC.normalise64(cam)
    assert peak[0] == 0.0 and not n.any() and np.isfinite(n).all()
    assert not GC.upsample64(n, 88, 200).any()


def test_heat_u8_rounding():
    h = np.array([0.0, 0.0019, 0.00197, 0.5, 0.998, 1.0], dtype=np.float32)
    assert GC.heat_u8_of(h).tolist() == [0, 0, 1, 128, 254, 255]


def _bare_predictor(batch=1, half=False):
    """A Predictor that owns no device state: enough for the checks that come before any launch
    (anything past them would fail on the missing engine)."""
    from cilrs_mi355.predict import Predictor
    p = object.__new__(Predictor)
    p.batch, p.half = batch, half
    p.frames_host = torch.zeros(batch, 88, 200, 3, dtype=torch.uint8)
    p.model = types.SimpleNamespace(num_commands=4)
    return p


def test_predictor_gradcam_argument_checks_need_no_device():
    p = _bare_predictor()
    u8 = np.zeros((1, 88, 200, 3), dtype=np.uint8)
    for kw in (dict(output="steering"), dict(output=(1.0, 2.0, 3.0)),
               dict(output=(1.0, 2.0, 3.0, float("nan"))), dict(layer="layer5"), dict(layer=4),
               dict(layer="avgpool")):
        with pytest.raises(ValueError):
            p.gradcam(u8, [10.0], [1], **kw)
    for frames, kmh, cmds in ((u8.astype(np.float32), [10.0], [1]), (u8[0], [10.0], [1]),
                              (np.zeros((2, 88, 200, 3), np.uint8), [10.0], [1]),
                              (np.zeros((1, 88, 200, 2), np.uint8), [10.0], [1]),
                              (u8, [10.0, 20.0], [1]), (u8, [10.0], [1, 2]), (u8, [10.0], [4]),
                              (u8, [10.0], [-1])):
        with pytest.raises(RuntimeError):
            p.gradcam(frames, kmh, cmds)
    with pytest.raises(RuntimeError, match="fp32 predictors only"):
        _bare_predictor(half=True).gradcam(u8, [10.0], [1])
    # camera-sized frames at layer4 are the single-frame path
    p2 = _bare_predictor(batch=2)
    with pytest.raises(RuntimeError, match="single-frame"):
        p2.gradcam(np.zeros((2, 60, 80, 4), np.uint8), [10.0, 20.0], [1, 2])
    # a valid call gets past the checks and only then misses the engine
    with pytest.raises(AttributeError):
        p.gradcam(u8, [10.0], [1])
