"""Viewpoint on the device: `cilrs_augment_view_u8` and `cilrs_batch_assemble_view` against the
float32 restatement in tests/_view.py (bit for bit: the warp is defined operation by operation),
against the weather / plain entry points (off records; fused == composed), the corrected labels,
through both loaders, inside guard bands, and through `evaluate.view_sweep`."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _view as VW
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


CASES = ("off", "identity", "integer translation", "half-pixel translation", "yaw only",
         "lateral only", "both", "translation by 10 W")


def _small_case():
    """B=8 at 9x11 (odd, no multiple of anything, split row 4 inside the frame), one record each"""
    from cilrs_mi355 import data as D
    B, h, w = 8, 9, 11
    frames = np.random.default_rng(1).integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    v = D.identity_view(B)
    v[1:2] = VW.translation(0.0, 0.0)
    v[2:3] = VW.translation(2.0, -1.0)
    v[3:4] = VW.translation(0.5, 0.5)
    v[4:5] = D.view_records(0.0, np.radians(5.0), 0.5, h, w)
    v[5:6] = D.view_records(0.5, 0.0, 0.5, h, w)
    v[6:7] = D.view_records(-0.5, np.radians(-5.0), 0.5, h, w)
    v[7:8] = VW.translation(10.0 * w, 0.0)
    v["split_row"] = (h - 1) / 2
    D.check_view(v, h, w)
    return frames, v


def test_view_kernel_matches_restatement_stage_by_stage():
    from cilrs_mi355 import data as D
    frames, v = _small_case()
    B, h, w = frames.shape[:3]
    want = VW.view_batch(frames, v)
    # the cases are what their names say
    assert np.array_equal(want[0], frames[0]) and np.array_equal(want[1], frames[1])
    assert np.array_equal(want[2][1:, :9], frames[2][:-1, 2:])
    assert np.array_equal(want[5][:5], frames[5][:5]), "lateral only: the far rows do not move"
    assert not np.array_equal(want[5][5:], frames[5][5:]), "lateral only: the ground rows move"
    assert np.array_equal(want[7], np.broadcast_to(frames[7][:, -1:], frames[7].shape))
    for b in range(2, B):
        assert not np.array_equal(want[b], frames[b]), CASES[b]
    dev = torch.from_numpy(frames).cuda()
    got = D.view_u8(dev, v).cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], want[b]), CASES[b]
    # with the stages behind it: blur 3 / 5 (taps through reflect-101 read V), colour, a hole
    p = D.identity_params(B)
    p["blur_k"][3], p["blur_w"][3] = 3, D.gaussian_taps(3, 0.8)
    p["blur_k"][4], p["blur_w"][4] = 5, D.gaussian_taps(5, 1.1)
    p["blur_k"][6], p["blur_w"][6] = 5, D.gaussian_taps(5, 2.0)
    p["rbc_on"][5], p["alpha"][5], p["beta255"][5] = 1, 1.15, -9.0
    p["hsv_on"][6], p["hue"][6], p["sat"][6], p["val"][6] = 1, 7.0, -12.0, 9.0
    p["nholes"][2] = 1
    p["hole_y0"][2, 0], p["hole_x0"][2, 0], p["hole_y1"][2, 0], p["hole_x1"][2, 0] = 2, 3, 5, 9
    img, out8 = D.augment_u8(dev, p, want_u8=True, view=v)
    want8, wantf = VW.augment_view_batch(frames, p, None, v)
    got8, gotf = out8.cpu().numpy(), img.permute(0, 2, 3, 1).cpu().numpy()
    for b in range(B):
        assert np.array_equal(got8[b], want8[b]), CASES[b]
        assert np.array_equal(gotf[b], wantf[b]), CASES[b]
    # and with weather between the two: rain and fog live in the image the network sees
    wx = D.WeatherMix(NO_CLEAR).draw(np.random.default_rng(3), B, h, w)
    img, out8 = D.augment_u8(dev, p, want_u8=True, weather=wx, view=v)
    want8, wantf = VW.augment_view_batch(frames, p, wx, v)
    assert np.array_equal(out8.cpu().numpy(), want8)
    assert np.array_equal(img.permute(0, 2, 3, 1).cpu().numpy(), wantf)


def _reference_case():
    """B=8 at 88x200: the mix's extremes and four drawn records, each sample under another weather,
    blur 3 and 5 on: the composition with the most taps"""
    from cilrs_mi355 import data as D
    B = 8
    frames = np.random.default_rng(4).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    frames[1] = np.random.default_rng(5).integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8) \
        .repeat(8, 0).repeat(8, 1)                                  # blocks: edges to interpolate
    spd = np.linspace(0.0, 1.0, B)
    v = D.ViewShift(p=1.0).draw(np.random.default_rng(31), B, spd, H, W)
    v[:4] = D.view_records([0.5, -0.5, 0.5, -0.5], np.radians([5.0, 5.0, -5.0, -5.0]), spd[:4],
                           H, W)
    assert (v["on"] == 1).all()
    names = ["clear", "fog", "night", "rain", "hardrain", "fog", "rain", "hardrain"]
    sev = [1.0, 1.0, 1.0, 1.0, 1.0, 0.4, 0.5, 0.6]
    rng = np.random.default_rng(32)
    wx = np.concatenate([D.weather_condition(nm, s, 1, H, rng) for nm, s in zip(names, sev)])
    assert len({r.tobytes() for r in wx}) == B
    p = D.identity_params(B)
    for b in range(B):
        k = 3 if b % 2 == 0 else 5
        p["blur_k"][b], p["blur_w"][b] = k, D.gaussian_taps(k, 0.7 + 0.3 * b)
    p["rbc_on"][2], p["alpha"][2], p["beta255"][2] = 1, 0.9, 12.0
    p["hsv_on"][5], p["hue"][5], p["sat"][5], p["val"][5] = 1, -6.0, 15.0, -8.0
    D.check_view(v, H, W)
    D.check_weather(wx, H, W)
    return frames, p, wx, v


def test_view_kernel_matches_restatement_on_the_reference_frame():
    from cilrs_mi355 import data as D
    frames, p, wx, v = _reference_case()
    dev = torch.from_numpy(frames).cuda()
    img, out8 = D.augment_u8(dev, p, want_u8=True, weather=wx, view=v)
    want8, wantf = VW.augment_view_batch(frames, p, wx, v)
    got8, gotf = out8.cpu().numpy(), img.permute(0, 2, 3, 1).cpu().numpy()
    for b in range(len(frames)):
        assert np.array_equal(got8[b], want8[b]), b
        assert np.array_equal(gotf[b], wantf[b]), b
    shown = VW.view_batch(frames, v)
    assert np.array_equal(D.view_u8(dev, v).cpu().numpy(), shown)
    assert (shown != frames).mean() > 0.5


def _cache(n, seed=2, h=H, w=W):
    from cilrs_mi355 import data as D
    g = torch.Generator().manual_seed(seed)
    cache = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g).cuda()
    speed = torch.rand(n, generator=g)
    command = torch.randint(0, 4, (n,), generator=g).cuda()
    targets = torch.rand(n, 3, generator=g)
    targets[:, 0] = targets[:, 0] * 2 - 1
    targets[0, 0], targets[5, 0], targets[12 % n, 0], targets[3, 0] = 0.99, -1.0, -0.0, 1.0
    return D.DeviceDataset.from_tensors(cache, speed.cuda(), command, targets.cuda())


INDEX = np.array([12, 5, 0, 9, 5, 12, 3, 1, 0, 7, 5])          # repeats, unordered, 8 + a short 3


def test_off_records_equal_the_other_entry_points():
    from cilrs_mi355 import data as D
    ds = _cache(13)
    assert np.signbit(ds.targets[12, 0].item()) and ds.targets[12, 0].item() == 0   # a stored -0.0
    p = D.draw_aug_params(np.random.default_rng(16), 16)[:len(INDEX)]
    off = D.view_records(0.5, np.radians(5.0), np.full(len(INDEX), 0.3), H, W)
    off["on"], off["steer_delta"] = 0, 0.5            # a real motion, switched off: none of it is read
    wx = D.WeatherMix(NO_CLEAR).draw(np.random.default_rng(5), len(INDEX), H, W)
    sel = torch.from_numpy(INDEX).cuda()
    for weather in (None, wx):
        want_img, want8 = D.augment_u8(ds.cache[sel], p, want_u8=True, weather=weather)
        img, out8 = D.augment_u8(ds.cache[sel], p, want_u8=True, weather=weather, view=off)
        assert torch.equal(img, want_img) and torch.equal(out8, want8)
        plain = ds.assemble(INDEX, p, want_u8=True, weather=weather)
        fused = ds.assemble(INDEX, p, want_u8=True, weather=weather, view=off)
        assert len(plain) == len(fused) == 5
        for a, b in zip(plain, fused):
            assert a.dtype == b.dtype and a.stride() == b.stride() and torch.equal(a, b)
        # bit for bit: the -0.0 steer of frame 12 is copied, never added to
        assert fused[3].cpu().numpy().tobytes() == plain[3].cpu().numpy().tobytes()
        assert np.signbit(fused[3][0, 0].item())
    assert torch.equal(D.view_u8(ds.cache[sel], off), ds.cache[sel])


def test_fused_assemble_equals_view_then_weather_then_augment():
    from cilrs_mi355 import data as D
    ds = _cache(13)
    p = D.draw_aug_params(np.random.default_rng(16), 16)[:len(INDEX)]
    assert (p["blur_k"] > 1).any() and p["hsv_on"].any() and (p["nholes"] > 0).any()
    wx = D.WeatherMix(NO_CLEAR).draw(np.random.default_rng(5), len(INDEX), H, W)
    v = D.ViewShift(p=0.8).draw(np.random.default_rng(6), len(INDEX), ds.speed_host[INDEX], H, W)
    assert 0 < (v["on"] == 0).sum() < len(INDEX)
    # INDEX[2] is frame 0 (steer 0.99) and INDEX[1] frame 5 (steer -1.0): push both over the clip
    v[2:3] = D.view_records(-0.5, np.radians(-5.0), ds.speed_host[0], H, W)
    v[1:2] = D.view_records(0.5, np.radians(5.0), ds.speed_host[5], H, W)
    assert v["steer_delta"][2] > 0.01 and v["steer_delta"][1] < 0
    targets = ds.targets.cpu().numpy()
    for weather in (wx, None):
        for lo, hi in ((0, 8), (8, 11)):                        # a full batch and a short last one
            idx, pb, vb = INDEX[lo:hi], p[lo:hi], v[lo:hi]
            wb = None if weather is None else weather[lo:hi]
            sel = torch.from_numpy(idx).cuda()
            img, spd, cmd, tgt, out8 = ds.assemble(idx, pb, want_u8=True, weather=wb, view=vb)
            shown = D.view_u8(ds.cache[sel], vb)
            assert not torch.equal(shown, ds.cache[sel])
            if wb is not None:
                shown = D.weather_u8(shown, wb)
            want_img, want8 = D.augment_u8(shown, pb, want_u8=True)
            assert img.shape == (hi - lo, 3, H, W) and img.stride() == want_img.stride()
            assert torch.equal(img, want_img) and torch.equal(out8, want8)
            # augment_u8 with the same records is the same launch on gathered frames
            img2, out82 = D.augment_u8(ds.cache[sel], pb, want_u8=True, weather=wb, view=vb)
            assert torch.equal(img2, want_img) and torch.equal(out82, want8)
            # labels: steer corrected and clipped, the rest untouched
            want_t = VW.correct_steer(targets[idx], vb)
            got_t = tgt.cpu().numpy()
            assert got_t.tobytes() == want_t.tobytes()
            assert got_t.tobytes() == D.correct_steer(targets[idx], vb).tobytes()
            assert np.array_equal(got_t[:, 1:], targets[idx][:, 1:])
            on = vb["on"] == 1
            assert np.array_equal(got_t[~on], targets[idx][~on])
            if lo == 0:
                assert got_t[2, 0] == 1.0 and got_t[1, 0] == -1.0   # 0.99 + delta, -1 - delta
                assert (got_t[on, 0] != targets[idx][on, 0]).sum() >= on.sum() - 2
            assert torch.equal(spd, ds.speed.index_select(0, sel))
            assert torch.equal(cmd, ds.command_dev.index_select(0, sel)) and cmd.dtype == torch.int64


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


@pytest.mark.parametrize("with_weather", [False, True])
def test_loaders_agree_with_a_view_mix(dataset, with_weather):
    from cilrs_mi355 import data as D
    s, tr_idx, va_idx, ds = dataset
    dev = torch.device("cuda")
    wx = (lambda: D.WeatherMix(NO_CLEAR)) if with_weather else (lambda: None)
    for idx, bs, train in ((tr_idx, 4, True), (va_idx, 4, False)):
        with D.BatchLoader(s, idx, bs, dev, train, seed=5, weather=wx(), view=D.ViewShift()) as a:
            b = D.CachedBatchLoader(ds, idx, bs, train, seed=5, weather=wx(), view=D.ViewShift())
            b0 = D.CachedBatchLoader(ds, idx, bs, train, seed=5, weather=wx())
            plan = D.CachedBatchLoader(ds, idx, bs, train, seed=5, weather=wx(),
                                       view=D.ViewShift())
            for epoch in range(2):
                with_a, with_b, off_b = _batches(a), _batches(b), _batches(b0)
                _assert_same(with_b, with_a, ("view", with_weather, train, epoch))
                view = plan.epoch_plan()[-1]
                moved = images = 0
                for bi, (x, y) in enumerate(zip(with_b, off_b)):
                    vb = view[bi * bs:bi * bs + len(x[0])]
                    on = torch.from_numpy(vb["on"] == 1).cuda()
                    # same order, speed, command, throttle and brake; steer by the record
                    assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])
                    want_t = D.correct_steer(y[3].cpu().numpy(), vb)
                    assert x[3].cpu().numpy().tobytes() == want_t.tobytes()
                    # off samples are the other loader's, on samples are seen from elsewhere
                    assert torch.equal(x[0][~on], y[0][~on])
                    moved += int((x[3][:, 0] != y[3][:, 0]).sum())
                    images += sum(not torch.equal(i, j) for i, j in zip(x[0][on], y[0][on]))
                n_on = int((view["on"] == 1).sum())
                assert 0 < n_on < len(view) and images == n_on and moved > 0
            if not train:
                assert len(with_b[-1][0]) == len(va_idx) % 4 == 1       # a short last batch


def test_view_entry_points_inside_guard_bands():
    from cilrs_mi355 import _lib as L
    from cilrs_mi355 import data as D
    frames, v = _small_case()
    B, h, w_ = 4, 9, 11
    frames, v = frames[4:], v[4:]                       # yaw, lateral, both, every pixel on one edge
    p = D.identity_params(B)
    p["blur_k"][2], p["blur_w"][2] = 5, D.gaussian_taps(5, 1.1)
    wx = D.WeatherMix(NO_CLEAR).draw(np.random.default_rng(3), B, h, w_)
    U8 = torch.uint8
    checks = []

    def buf(shape, dtype, fill, guard, name):
        t, chk = guarded(int(np.prod(shape)), dtype, fill, guard, name)
        checks.append(chk)
        return t.view(shape)

    fr = torch.from_numpy(frames).cuda()
    pdev, wdev, vdev = _dev(p), _dev(wx), _dev(v)
    nan = float("nan")
    n = B
    speed, targets = torch.rand(n, device="cuda"), torch.rand(n, 3, device="cuda")
    command = torch.randint(0, 4, (n,), device="cuda")
    index = torch.tensor([3, 2, 1, 0], device="cuda")
    cache = fr.flip(0).contiguous()
    for weather, wptr in ((wx, wdev), (None, None)):
        tag = "view+weather" if weather is not None else "view"
        checks.clear()
        outf = buf((B, h, w_, 3), torch.float32, nan, h * w_ * 3, tag + " augment out_f32")
        out8 = buf((B, h, w_, 3), U8, 7, h * w_ * 3, tag + " augment out_u8")
        ins = Inputs(frames=fr, params=pdev, weather=wdev, view=vdev)
        L.check(L.lib().cilrs_augment_view_u8(L.ptr(fr), L.ptr(pdev), L.ptr(wptr), L.ptr(vdev), B,
                                              h, w_, L.ptr(outf), L.ptr(out8), _stream()))
        for chk in checks:
            chk()
        ins.check()
        all_finite(outf, tag + " augment out_f32")
        want8, wantf = VW.augment_view_batch(frames, p, weather, v)
        assert np.array_equal(out8.cpu().numpy(), want8)
        assert np.array_equal(outf.cpu().numpy(), wantf)
        # cilrs_batch_assemble_view over a cache of the same four frames, reversed
        checks.clear()
        asf = buf((B, h, w_, 3), torch.float32, nan, h * w_ * 3, tag + " assemble out_f32")
        as8 = buf((B, h, w_, 3), U8, 7, h * w_ * 3, tag + " assemble out_u8")
        ospd = buf((B,), torch.float32, nan, B, tag + " assemble out_speed")
        ocmd = buf((B,), torch.int64, -1, B, tag + " assemble out_command")
        otgt = buf((B, 3), torch.float32, nan, 3 * B, tag + " assemble out_targets")
        ins = Inputs(cache=cache, speed=speed, command=command, targets=targets, index=index,
                     params=pdev, weather=wdev, view=vdev)
        L.check(L.lib().cilrs_batch_assemble_view(
            L.ptr(cache), n, L.ptr(speed), L.ptr(command), L.ptr(targets), L.ptr(index),
            L.ptr(pdev), L.ptr(wptr), L.ptr(vdev), B, h, w_, L.ptr(asf), L.ptr(as8), L.ptr(ospd),
            L.ptr(ocmd), L.ptr(otgt), _stream()))
        for chk in checks:
            chk()
        ins.check()
        for t, name in ((asf, "out_f32"), (ospd, "out_speed"), (otgt, "out_targets")):
            all_finite(t, tag + " assemble " + name)
        assert torch.equal(as8, out8) and torch.equal(asf, outf) and int(ocmd.min()) >= 0
        assert torch.equal(ospd, speed.flip(0)) and torch.equal(ocmd, command.flip(0))
        want_t = VW.correct_steer(targets.flip(0).cpu().numpy(), v)
        assert otgt.cpu().numpy().tobytes() == want_t.tobytes()


def test_view_sweep_returns_every_cell():
    import inspect
    from cilrs_mi355 import CILRS
    from cilrs_mi355 import data as D
    from cilrs_mi355 import evaluate as E
    sig = inspect.signature(E.view_sweep).parameters
    assert tuple(sig["lateral_m"].default) == (-1, -0.5, 0, 0.5, 1)
    assert tuple(sig["yaw_deg"].default) == (-6, -3, 0, 3, 6)
    assert sig["weather"].default is None and sig["batch_size"].default == 128
    ds = _cache(16, seed=9)
    idx = np.arange(16)
    m = CILRS(4, dropout=0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0), strict=True)
    m = m.cuda().eval()
    lats, yaws = (-0.5, 0.0, 0.5), (-4.0, 0.0, 4.0)
    rep = E.view_sweep(m, ds, idx, lateral_m=lats, yaw_deg=yaws, batch_size=8)
    assert set(rep) == {"centre", "cells", "slopes"} and set(rep["cells"]) == set(lats)
    dump = lambda r: json.dumps(r, sort_keys=True)
    plain = E.evaluate(m, D.CachedBatchLoader(ds, idx, 8, train=False))
    assert dump(rep["centre"]) == dump(plain) and plain["val_samples"] == 16
    spd = ds.speed_host[idx]
    for lat in lats:
        assert set(rep["cells"][lat]) == set(yaws)
        for yaw in yaws:
            cell = rep["cells"][lat][yaw]
            assert set(cell) == {"report", "steer_mae", "steer_shift", "steer_delta", "gain"}
            assert cell["report"]["val_samples"] == 16
            assert cell["steer_mae"] == cell["report"]["overall_metrics"]["Steer"]["MAE"]
            want = D.view_records(lat, np.radians(yaw), spd, H, W)["steer_delta"]
            assert cell["steer_delta"] == pytest.approx(float(want.mean(dtype=np.float64)), abs=1e-7)
            if (lat, yaw) == (0.0, 0.0):
                assert cell["steer_delta"] == 0 and cell["gain"] is None
            else:
                assert cell["gain"] == cell["steer_shift"] / cell["steer_delta"]
    centre = rep["cells"][0.0][0.0]
    assert dump(centre["report"]) == dump(plain) and centre["steer_shift"] == 0.0
    xs = np.array(lats)
    ys = np.array([rep["cells"][v][0.0]["steer_shift"] for v in lats])
    assert rep["slopes"]["steer_per_m"] == pytest.approx(np.polyfit(xs, ys, 1)[0], abs=1e-12)
    ys = np.array([rep["cells"][0.0][v]["steer_shift"] for v in yaws])
    assert rep["slopes"]["steer_per_deg"] == pytest.approx(np.polyfit(np.array(yaws), ys, 1)[0],
                                                           abs=1e-12)
    json.dumps(rep)                                                    # what the JSON twin writes
    # a displaced cell's inputs and labels are not the centre's
    v = D.ViewShift.fixed(0.5, 4.0).draw(np.random.default_rng(0), 16, spd, H, W)
    assert (D.view_u8(ds.cache, v) != ds.cache).float().mean() > 0.5
    assert rep["cells"][0.5][4.0]["steer_delta"] < 0 < rep["cells"][-0.5][-4.0]["steer_delta"]
