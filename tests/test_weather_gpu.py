"""Weather on the device: `cilrs_augment_weather_u8` and `cilrs_batch_assemble_weather` against the
float32 restatement in tests/_weather.py (bit for bit: nothing transcendental runs on the device),
against the plain entry points (identity records; fused == composed), through both loaders, inside
guard bands, and through `evaluate.weather_sweep`."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _weather as WX
import cilrs_oracle as O
from _guards import Inputs, all_finite, guarded
from test_host import make_sessions

pytestmark = pytest.mark.gpu

H, W = 88, 200
NO_CLEAR = {"fog": .25, "night": .25, "rain": .25, "hardrain": .25}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), -1)).cuda()


def _rain(w, i, slant, seed, p=0.03, length=16):
    w["rain_len"][i], w["rain_slant_q4"][i], w["rain_seed"][i] = length, slant, seed
    w["rain_thresh24"][i], w["rain_alpha"][i], w["rain_v255"][i] = int(p * (1 << 24)), 0.6, 215.0


def _fog(D, w, i, beta, h):
    w["fog_on"][i] = 1
    w["fog_t0"][i], w["fog_t1"][i] = D.fog_transmission(beta, h)
    w["fog_horizon"][i], w["fog_near"][i] = D.FOG_HORIZON * h, D.FOG_NEAR * h
    w["fog_rgb255"][i] = (200, 205, 210)


def _tone(w, i):
    w["tone_on"][i], w["gain"][i], w["lift255"][i] = 1, (0.7, 0.8, 1.2), (5.0, -3.0, 0.0)


def _small_case():
    """B=6 at 9x13, one stage per sample: the frame is smaller than a 16-long streak, so heads
    above and beside it decide pixels, and the blur's reflect border meets weather taps."""
    from cilrs_mi355 import data as D
    B, h, w_ = 6, 9, 13
    frames = np.random.default_rng(1).integers(0, 256, (B, h, w_, 3), dtype=np.uint8)
    frames[0, 0:2], frames[0, 2:4], frames[0, 4:6] = 0, 255, 128
    w = D.identity_weather(B)
    _tone(w, 0)
    _fog(D, w, 1, 1.9, h)
    _rain(w, 2, 16, 11)
    _rain(w, 3, -16, 12)
    for i in (4, 5):                                   # everything at once
        _tone(w, i)
        _fog(D, w, i, 0.9, h)
        _rain(w, i, 5 if i == 4 else -7, 13 + i, p=0.05, length=11)
    p = D.identity_params(B)
    p["blur_k"][5], p["blur_w"][5] = 5, D.gaussian_taps(5, 1.1)
    p["nholes"][5] = 1
    p["hole_y0"][5, 0], p["hole_x0"][5, 0], p["hole_y1"][5, 0], p["hole_x1"][5, 0] = 2, 3, 5, 9
    D.check_weather(w, h, w_)
    return frames, p, w


def test_weather_kernel_matches_restatement_stage_by_stage():
    from cilrs_mi355 import data as D
    frames, p, w = _small_case()
    B, h, w_ = frames.shape[:3]
    for i in (2, 3):                                   # heads off the frame do decide pixels here
        jmin = WX.rain_cover(w[i], h, w_)
        y, x = np.nonzero(jmin < 16)
        hy, hx = y - jmin[y, x], x - ((jmin[y, x] * int(w["rain_slant_q4"][i])) >> 4)
        assert ((hy < 0) | (hx < 0) | (hx >= w_)).any() and (jmin == 16).any(), i
    img, out8 = D.augment_u8(torch.from_numpy(frames).cuda(), p, want_u8=True, weather=w)
    want8, wantf = WX.augment_weather_batch(frames, p, w)
    got8 = out8.cpu().numpy()
    for b in range(B):
        assert not np.array_equal(want8[b], frames[b]), f"sample {b}: the weather did nothing"
        assert np.array_equal(got8[b], want8[b]), f"sample {b}"
    assert img.shape == (B, 3, h, w_)
    assert np.array_equal(img.permute(0, 2, 3, 1).cpu().numpy(), wantf)
    # weather_u8 is the weather alone
    only = D.weather_u8(torch.from_numpy(frames).cuda(), w)
    assert np.array_equal(only.cpu().numpy(), WX.weather_batch(frames, w))


def _reference_case():
    from cilrs_mi355 import data as D
    B = 4
    frames = np.random.default_rng(4).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    w = D.WeatherMix(NO_CLEAR).draw(np.random.default_rng(21), B, H, W)
    assert (w["rain_len"] > 0).any() and (w["fog_on"] == 1).any() and (w["tone_on"] == 1).all()
    p16 = D.draw_aug_params(np.random.default_rng(16), 16)
    first = lambda m: int(np.nonzero(m)[0][0])
    p = p16[[first(p16["hsv_on"]), first(p16["blur_k"] == 5), first(p16["nholes"] > 0),
             first(p16["rbc_on"])]].copy()
    rainy = int(np.nonzero(w["rain_len"] > 0)[0][-1])
    if p["blur_k"][rainy] == 0:                                           # blur over rainy taps
        p["blur_k"][rainy], p["blur_w"][rainy] = 3, D.gaussian_taps(3, 1.0)
    assert (p["blur_k"][w["rain_len"] > 0] > 1).sum() >= 2
    return frames, p, w


def test_weather_kernel_matches_restatement_on_the_reference_frame():
    from cilrs_mi355 import data as D
    frames, p, w = _reference_case()
    dev = torch.from_numpy(frames).cuda()
    quiet = p.copy()
    quiet["noise_std255"], quiet["noise_seed"] = 0.0, 0
    img, out8 = D.augment_u8(dev, quiet, want_u8=True, weather=w)
    want8, wantf = WX.augment_weather_batch(frames, quiet, w)
    assert np.array_equal(out8.cpu().numpy(), want8)
    assert np.array_equal(img.permute(0, 2, 3, 1).cpu().numpy(), wantf)
    # with noise: logf / cosf differ from numpy's by an ulp, so a grey level may flip, rarely
    noisy = p.copy()
    noisy["noise_std255"] = (5.1, 0.0, 10.2, 15.3)
    noisy["noise_seed"] = (123456789, 0, 42, 7)
    _, out8 = D.augment_u8(dev, noisy, want_u8=True, weather=w)
    want8, _ = WX.augment_weather_batch(frames, noisy, w)
    diff = np.abs(out8.cpu().numpy().astype(int) - want8.astype(int))
    assert diff.max() <= 1
    for b in range(len(frames)):
        if noisy["noise_std255"][b] == 0:
            assert diff[b].max() == 0, b
        else:
            assert (diff[b] > 0).mean() <= 2e-3, b


def _cache(n, seed=2):
    from cilrs_mi355 import data as D
    g = torch.Generator().manual_seed(seed)
    cache = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    speed = torch.rand(n, generator=g).cuda()
    command = torch.randint(0, 4, (n,), generator=g).cuda()
    targets = torch.rand(n, 3, generator=g).cuda()
    return D.DeviceDataset.from_tensors(cache, speed, command, targets)


INDEX = np.array([12, 5, 0, 9, 5, 12, 3, 1, 0, 7, 5])          # repeats, unordered, 8 + a short 3


def test_identity_weather_equals_the_plain_entry_points():
    from cilrs_mi355 import data as D
    ds = _cache(13)
    p = D.draw_aug_params(np.random.default_rng(16), 16)[:len(INDEX)]
    off = D.identity_weather(len(INDEX))
    sel = torch.from_numpy(INDEX).cuda()
    want_img, want8 = D.augment_u8(ds.cache[sel], p, want_u8=True)
    img, out8 = D.augment_u8(ds.cache[sel], p, want_u8=True, weather=off)
    assert torch.equal(img, want_img) and torch.equal(out8, want8)
    assert torch.equal(D.weather_u8(ds.cache[sel], off), ds.cache[sel])
    plain = ds.assemble(INDEX, p, want_u8=True)
    fused = ds.assemble(INDEX, p, want_u8=True, weather=off)
    assert len(plain) == len(fused) == 5
    for a, b in zip(plain, fused):
        assert a.dtype == b.dtype and a.stride() == b.stride() and torch.equal(a, b)


def test_fused_assemble_equals_weather_then_augment():
    from cilrs_mi355 import data as D
    ds = _cache(13)
    p = D.draw_aug_params(np.random.default_rng(16), 16)[:len(INDEX)]
    assert (p["blur_k"] > 1).any() and p["hsv_on"].any() and (p["nholes"] > 0).any()
    w = D.WeatherMix(NO_CLEAR).draw(np.random.default_rng(5), len(INDEX), H, W)
    for lo, hi in ((0, 8), (8, 11)):                            # a full batch and a short last one
        idx, pb, wb = INDEX[lo:hi], p[lo:hi], w[lo:hi]
        sel = torch.from_numpy(idx).cuda()
        img, spd, cmd, tgt, out8 = ds.assemble(idx, pb, want_u8=True, weather=wb)
        shown = D.weather_u8(ds.cache[sel], wb)
        assert not torch.equal(shown, ds.cache[sel])
        want_img, want8 = D.augment_u8(shown, pb, want_u8=True)
        assert img.shape == (hi - lo, 3, H, W) and img.stride() == want_img.stride()
        assert torch.equal(img, want_img) and torch.equal(out8, want8)
        assert torch.equal(spd, ds.speed.index_select(0, sel))
        assert torch.equal(cmd, ds.command_dev.index_select(0, sel)) and cmd.dtype == torch.int64
        assert torch.equal(tgt, ds.targets.index_select(0, sel))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from cilrs_mi355 import data as D
    root = str(tmp_path_factory.mktemp("sessions"))
    make_sessions(root, (14, 13))
    s = D.Sessions(root)
    tr_idx, va_idx = s.split()
    return s, tr_idx, va_idx, D.DeviceDataset(s, "cuda", workers=3, chunk_frames=5)


def _batches(loader):
    return [[t.clone() for t in batch] for batch in loader]


def _assert_same(got, want, what):
    assert len(got) == len(want) > 0, what
    for bi, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 4
        for k, (a, b) in enumerate(zip(g, w)):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, bi, k)


def test_loaders_agree_with_a_mix_and_without(dataset):
    from cilrs_mi355 import data as D
    s, tr_idx, va_idx, ds = dataset
    dev = torch.device("cuda")
    for idx, bs, train in ((tr_idx, 4, True), (va_idx, 4, False)):
        mix = D.WeatherMix(NO_CLEAR)
        plain_plan = D.CachedBatchLoader(ds, idx, bs, train, seed=5)
        with D.BatchLoader(s, idx, bs, dev, train, seed=5, weather=mix) as a, \
                D.BatchLoader(s, idx, bs, dev, train, seed=5) as a0:
            b = D.CachedBatchLoader(ds, idx, bs, train, seed=5, weather=mix)
            b0 = D.CachedBatchLoader(ds, idx, bs, train, seed=5)
            for epoch in range(2):
                with_a, with_b = _batches(a), _batches(b)
                _assert_same(with_b, with_a, ("mix", train, epoch))
                off_a, off_b = _batches(a0), _batches(b0)
                _assert_same(off_b, off_a, ("off", train, epoch))
                # weather=None is the parent's loader: the plain entry point on the same plan
                order, params = plain_plan.epoch_plan()
                for bi, got in enumerate(off_b):
                    ids = order[bi * bs:(bi + 1) * bs]
                    sel = torch.from_numpy(ids).cuda()
                    want = D.augment_u8(ds.cache[sel], params[bi * bs:bi * bs + len(ids)])
                    assert torch.equal(got[0], want), (train, epoch, bi)
                    assert torch.equal(got[2], ds.command_dev.index_select(0, sel))
                # same order and labels with the mix; the images differ
                for x, y in zip(with_b, off_b):
                    assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])
                assert any(not torch.equal(x[0], y[0]) for x, y in zip(with_b, off_b))
            if not train:
                assert len(with_b[-1][0]) == len(va_idx) % 4 == 1       # a short last batch


def test_weather_entry_points_inside_guard_bands():
    from cilrs_mi355 import _lib as L
    frames, p, w = _small_case()
    B, h, w_ = 3, 9, 13
    frames, p, w = frames[3:], p[3:], w[3:]                    # rain -16, all, all + blur + hole
    U8 = torch.uint8
    checks, consts = [], {}

    def buf(shape, dtype, fill, guard, name):
        v, chk = guarded(int(np.prod(shape)), dtype, fill, guard, name)
        checks.append(chk)
        return v.view(shape)

    fr = torch.from_numpy(frames).cuda()
    pdev, wdev = _dev(p), _dev(w)
    nan = float("nan")
    # cilrs_augment_weather_u8
    outf = buf((B, h, w_, 3), torch.float32, nan, h * w_ * 3, "augment_weather out_f32")
    out8 = buf((B, h, w_, 3), U8, 7, h * w_ * 3, "augment_weather out_u8")
    ins = Inputs(frames=fr, params=pdev, weather=wdev)
    L.check(L.lib().cilrs_augment_weather_u8(L.ptr(fr), L.ptr(pdev), L.ptr(wdev), B, h, w_,
                                             L.ptr(outf), L.ptr(out8), _stream()))
    for chk in checks:
        chk()
    ins.check()
    all_finite(outf, "augment_weather out_f32")
    want8, wantf = WX.augment_weather_batch(frames, p, w)
    assert np.array_equal(out8.cpu().numpy(), want8) and np.array_equal(outf.cpu().numpy(), wantf)
    # cilrs_batch_assemble_weather over a cache of the same three frames, reversed
    checks.clear()
    n = B
    speed, targets = torch.rand(n, device="cuda"), torch.rand(n, 3, device="cuda")
    command = torch.randint(0, 4, (n,), device="cuda")
    index = torch.tensor([2, 1, 0], device="cuda")
    asf = buf((B, h, w_, 3), torch.float32, nan, h * w_ * 3, "assemble_weather out_f32")
    as8 = buf((B, h, w_, 3), U8, 7, h * w_ * 3, "assemble_weather out_u8")
    ospd = buf((B,), torch.float32, nan, B, "assemble_weather out_speed")
    ocmd = buf((B,), torch.int64, -1, B, "assemble_weather out_command")
    otgt = buf((B, 3), torch.float32, nan, 3 * B, "assemble_weather out_targets")
    cache = fr.flip(0).contiguous()
    ins = Inputs(cache=cache, speed=speed, command=command, targets=targets, index=index,
                 params=pdev, weather=wdev)
    L.check(L.lib().cilrs_batch_assemble_weather(
        L.ptr(cache), n, L.ptr(speed), L.ptr(command), L.ptr(targets), L.ptr(index), L.ptr(pdev),
        L.ptr(wdev), B, h, w_, L.ptr(asf), L.ptr(as8), L.ptr(ospd), L.ptr(ocmd), L.ptr(otgt),
        _stream()))
    for chk in checks:
        chk()
    ins.check()
    for t, name in ((asf, "out_f32"), (ospd, "out_speed"), (otgt, "out_targets")):
        all_finite(t, "assemble_weather " + name)
    assert torch.equal(as8, out8) and torch.equal(asf, outf) and int(ocmd.min()) >= 0
    assert torch.equal(ospd, speed.flip(0)) and torch.equal(otgt, targets.flip(0))


def test_weather_sweep_returns_every_cell():
    import inspect
    from cilrs_mi355 import CILRS
    from cilrs_mi355 import data as D
    from cilrs_mi355 import evaluate as E
    sig = inspect.signature(E.weather_sweep).parameters
    assert tuple(sig["severities"].default) == (0.25, 0.5, 0.75, 1.0)
    assert sig["batch_size"].default == 128 and sig["seed"].default == 0
    ds = _cache(24, seed=9)
    idx = np.arange(24)
    m = CILRS(4, dropout=0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0), strict=True)
    m = m.cuda().eval()
    rep = E.weather_sweep(m, ds, idx, severities=(0.0, 1.0), batch_size=16)
    assert set(rep) == {"clear", "steer_mae"} | set(D.WEATHER_CONDITIONS[1:])
    dump = lambda r: json.dumps(r, sort_keys=True)
    clear = E.evaluate(m, D.CachedBatchLoader(ds, idx, 16, train=False))
    assert dump(rep["clear"]) == dump(clear) and clear["val_samples"] == 24
    for name in D.WEATHER_CONDITIONS[1:]:
        assert set(rep[name]) == {0.0, 1.0} == set(rep["steer_mae"][name])
        assert dump(rep[name][0.0]) == dump(clear), name               # severity 0 is clear
        assert rep[name][1.0]["val_samples"] == 24
        cell = rep["steer_mae"][name][1.0]
        assert cell["mae"] == rep[name][1.0]["overall_metrics"]["Steer"]["MAE"]
        assert cell["ratio_to_clear"] == cell["mae"] / rep["steer_mae"]["clear"]
        assert rep["steer_mae"][name][0.0]["ratio_to_clear"] == 1.0
    json.dumps(rep)                                                    # what the JSON twin writes
    # the hardrain cell's inputs are not the clear ones (an untrained net's metric proves nothing)
    w = D.WeatherMix.fixed("hardrain", 1.0).draw(np.random.default_rng(0), 24, H, W)
    shown = D.weather_u8(ds.cache, w)
    assert (shown != ds.cache).float().mean() > 0.5
