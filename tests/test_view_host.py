"""Viewpoint randomisation, host side: the record layout, the float32 restatement's own properties
(identity, clamp), the geometry of `view_records` against an independent float64 pinhole camera,
the steering rule, the record checks, the mix, the loaders' plans with a mix, and the C entries'
refusals.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _view as VW
from cilrs_mi355 import data as D
from test_device_dataset_host import LabelsOnly

H, W = D.IMG_HEIGHT, D.IMG_WIDTH


def _frame(seed=0, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_record_layout_and_exports():
    import cilrs_mi355
    from cilrs_mi355 import _lib as L
    assert D.VIEW_DTYPE.itemsize == 96                   # cilrs_view_params, include/cilrs_hip.h
    offsets = {k: D.VIEW_DTYPE.fields[k][1] for k in D.VIEW_DTYPE.names}
    assert offsets == {"on": 0, "split_row": 4, "far": 8, "ground": 44, "steer_delta": 80,
                       "lateral_m": 84, "yaw_rad": 88, "reserved": 92}
    # the header's struct, field by field in the same order, all 4-byte members
    header = os.path.join(os.path.dirname(__file__), "..", "include", "cilrs_hip.h")
    with open(header) as f:
        body = re.search(r"typedef struct \{([^}]*)\} cilrs_view_params;", f.read()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.split()[0] in ("int", "float"), decl
            names += [re.sub(r"\[\d+\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    assert tuple(names) == D.VIEW_DTYPE.names
    assert "float far[9], ground[9]" in body
    assert D.identity_view(3).dtype == D.VIEW_DTYPE and (D.identity_view(3)["on"] == 0).all()
    lib = L.lib()
    for sym in ("cilrs_augment_view_u8", "cilrs_batch_assemble_view"):
        assert getattr(lib, sym) is not None
    for name in ("ViewShift", "CameraModel", "view_records", "view_u8"):
        assert hasattr(cilrs_mi355, name)


def test_camera_is_the_references():
    fx, fy, cx, cy = D.CameraModel().intrinsics(H, W)
    assert abs(fx - 83.9) < 0.05 and abs(fy - 49.2) < 0.05 and (cx, cy) == (99.5, 43.5)
    assert np.allclose((fx, fy, cx, cy), VW.intrinsics(H, W), rtol=1e-12)
    assert abs(D.CameraModel().f0 - 400 / np.tan(np.radians(50))) < 1e-9


def test_zero_motion_is_the_identity_map():
    v = D.view_records(0.0, 0.0, [0.0, 0.3, 1.0], H, W)
    eye = np.eye(3, dtype=np.float32).reshape(9)
    assert (v["on"] == 1).all() and (v["split_row"] == (H - 1) / 2).all()
    assert (v["far"] == eye).all() and (v["ground"] == eye).all()
    assert (v["steer_delta"] == 0).all() and not np.signbit(v["steer_delta"]).any()
    # a lateral motion alone leaves the far map the identity, exactly
    v = D.view_records(0.4, 0.0, 0.5, H, W)
    assert (v["far"] == eye).all() and not (v["ground"] == eye).all()


@pytest.mark.parametrize("h,w", [(H, W), (9, 11)])
def test_identity_map_returns_the_bytes(h, w):
    f = _frame(1, h, w)
    v = D.identity_view(1)
    assert np.array_equal(VW.view_one(f, v[0]), f)                 # off
    v["on"] = 1
    sx, sy = VW.source_coords(v[0], h, w)                          # ax = ay = 0: p00 exactly
    assert np.array_equal(sx, np.broadcast_to(np.arange(w, dtype=np.float32), (h, w)))
    assert np.array_equal(sy, np.broadcast_to(np.arange(h, dtype=np.float32)[:, None], (h, w)))
    assert np.array_equal(VW.view_one(f, v[0]), f)
    assert np.array_equal(VW.view_one(f, D.view_records(0.0, 0.0, 0.5, h, w)[0]), f)


def test_translations_under_the_restatement():
    f = _frame(2, 9, 11)
    out = VW.view_one(f, VW.translation(2, -1)[0])                 # source = destination + (2, -1)
    assert np.array_equal(out[1:, :9], f[:-1, 2:])
    assert np.array_equal(out[0, :9], f[0, 2:]) and np.array_equal(out[3, 9:], f[2, [10, 10]])
    half = VW.view_one(f, VW.translation(0.5, 0.0)[0]).astype(int)
    mean = (f[:, :-1].astype(int) + f[:, 1:].astype(int)) / 2.0
    assert np.array_equal(half[:, :-1], np.rint(mean).astype(int))  # ties to even, as rintf
    assert np.array_equal(half[:, -1], f[:, -1])
    edge = VW.view_one(f, VW.translation(10 * 11, 0.0)[0])
    assert np.array_equal(edge, np.broadcast_to(f[:, -1:], f.shape))


MOTIONS = [(0.5, 0.0), (-0.5, 0.0), (0.0, 5.0), (0.0, -5.0), (0.5, 5.0), (-0.37, 2.2), (1.0, -6.0)]


@pytest.mark.parametrize("h,w", [(H, W), (9, 11)])
@pytest.mark.parametrize("lateral,yaw_deg", MOTIONS)
def test_maps_against_an_independent_pinhole_camera(lateral, yaw_deg, h, w):
    yaw = np.radians(yaw_deg)
    v = D.view_records(lateral, yaw, 0.5, h, w)[0]
    rng = np.random.default_rng(3)
    n = 200
    # ground points of the flat road 1.4 m under the camera
    Z = rng.uniform(2.0, 60.0, n)
    X = np.stack([rng.uniform(-0.6, 0.6, n) * Z, np.full(n, 1.4), Z], axis=1)
    src = VW.project(X, h, w)
    dst = VW.project(X, h, w, lateral, yaw)
    assert (dst[1] > (h - 1) / 2).all()                            # below the horizon: ground rows
    got = VW.apply_map(v["ground"], *dst)
    err = max(np.abs(got[0] - src[0]).max(), np.abs(got[1] - src[1]).max())
    print("ground map error %.2e px" % err)
    assert err <= 1e-3
    # directions (points at infinity) anywhere in front
    d = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n), np.ones(n)], axis=1)
    src = VW.project(d, h, w, at_infinity=True)
    dst = VW.project(d, h, w, lateral, yaw, at_infinity=True)
    got = VW.apply_map(v["far"], *dst)
    err = max(np.abs(got[0] - src[0]).max(), np.abs(got[1] - src[1]).max())
    print("far map error %.2e px" % err)
    assert err <= 1e-3
    # the two agree along the horizon row, which stays put
    px = np.arange(w, dtype=np.float64)
    py = np.full(w, (h - 1) / 2)
    a, b = VW.apply_map(v["far"], px, py), VW.apply_map(v["ground"], px, py)
    assert np.abs(a[0] - b[0]).max() <= 1e-3 and np.abs(a[1] - b[1]).max() <= 1e-3
    assert np.abs(a[1] - py).max() <= 1e-3
    # w = 1 at the principal point
    for name in ("far", "ground"):
        m = v[name].astype(np.float64)
        assert abs(m[6] * (w - 1) / 2 + m[7] * (h - 1) / 2 + m[8] - 1) <= 1e-6
    D.check_view(np.array([v]), h, w)


def test_steering_rule():
    t = np.array([0.5, -0.5, 0.0, 0.0, 0.3, 0.0])
    psi = np.radians([0.0, 0.0, 5.0, -5.0, -2.0, 0.0])
    spd = np.array([0.5, 0.5, 0.5, 0.5, 0.05, 0.9])
    v = D.view_records(t, psi, spd, H, W)
    sd = v["steer_delta"]
    # a camera moved right or yawed right steers left
    assert sd[0] < 0 < sd[1] and sd[2] < 0 < sd[3] and sd[0] == -sd[1] and sd[2] == -sd[3]
    assert sd[5] == 0 and v["lateral_m"][0] == np.float32(0.5)
    assert v["yaw_rad"][2] == np.float32(np.radians(5.0))
    # the formula, restated in float64
    want = []
    for ti, pi, si in zip(t, psi, spd):
        vel = si * 40 / 3.6
        look = max(1.0 * vel, 4.0)
        yt = -ti * np.cos(pi) - look * np.sin(pi)
        want.append(np.arctan(2.875 * 2 * yt / look ** 2) / np.radians(70))
    assert np.array_equal(sd, np.array(want, dtype=np.float32))
    assert max(1.0 * spd[4] * 40 / 3.6, 4.0) == 4.0               # the slow sample hits the floor
    # every assumption is an argument
    kw = dict(lookahead_s=0.5, min_lookahead_m=2.0, wheelbase_m=2.5, max_steer_deg=35.0)
    got = D.view_records(0.5, 0.02, 0.6, H, W, **kw)["steer_delta"][0]
    look = max(0.5 * 0.6 * 40 / 3.6, 2.0)
    yt = -0.5 * np.cos(0.02) - look * np.sin(0.02)
    assert got == np.float32(np.arctan(2.5 * 2 * yt / look ** 2) / np.radians(35.0))
    with pytest.raises(TypeError):
        D.view_records(0.5, 0.0, 0.5, H, W, look_ahead=1.0)
    mix = D.ViewShift.fixed(0.5, 0.02 * 180 / np.pi, **kw)
    # (the mix goes through degrees: one float64 rounding of the yaw away)
    assert abs(mix.draw(np.random.default_rng(0), 1, [0.6], H, W)["steer_delta"][0] - got) < 1e-6


def test_label_correction_clips_at_one():
    v = D.identity_view(5)
    v["on"] = (1, 1, 1, 0, 1)
    v["steer_delta"] = (0.05, -0.05, 0.25, 0.25, 0.0)
    tg = np.array([[0.99, .1, .2], [-1.0, .3, .4], [0.5, .5, .6], [-0.0, .7, .8], [-0.0, 0, 0]],
                  dtype=np.float32)
    got = D.correct_steer(tg, v)
    assert got.dtype == np.float32 and got.tobytes() == VW.correct_steer(tg, v).tobytes()
    assert got[0, 0] == 1 and got[1, 0] == -1 and got[2, 0] == np.float32(0.5) + np.float32(0.25)
    assert got[3, 0] == 0 and np.signbit(got[3, 0])                # off: copied, -0.0 stays
    assert np.array_equal(got[:, 1:], tg[:, 1:]) and tg[0, 0] == np.float32(0.99)


def _good():
    return D.view_records([0.3, -0.4], np.radians([2.0, -3.0]), [0.5, 0.2], H, W)


@pytest.mark.parametrize("field,value", [
    ("on", 2), ("on", -1), ("split_row", np.nan), ("split_row", -1.5), ("split_row", H + 0.5),
    ("far", np.nan), ("far", np.inf), ("ground", np.nan), ("ground", -np.inf),
    ("steer_delta", np.nan), ("steer_delta", 2.5), ("steer_delta", -2.5), ("lateral_m", np.inf),
    ("yaw_rad", np.nan)])
def test_check_view_refuses_each_bad_field(field, value):
    v = _good()
    D.check_view(v, H, W)
    if v[field].ndim == 2:
        v[field][1, 4] = value
    else:
        v[field][1] = value
    with pytest.raises(RuntimeError, match="view"):
        D.check_view(v, H, W)


def test_check_view_refuses_dtype_and_small_w():
    v = _good()
    with pytest.raises(RuntimeError, match="VIEW_DTYPE"):
        D.check_view(v.view(np.uint8), H, W)
    with pytest.raises(RuntimeError, match="VIEW_DTYPE"):
        D.check_view(D.identity_weather(2), H, W)
    D.check_view(v[:0], H, W)
    for edge in (-1.0, float(H)):                                   # the ends of the split range
        v["split_row"] = edge
        D.check_view(v, H, W)
    # +-10 degrees keeps w above 0.79 at 200x88; a yaw that drives a corner under 0.25 is refused
    ten = D.view_records(0.0, np.radians([10.0, -10.0]), 0.5, H, W)
    assert abs(D._view_w_min(ten, H, W).min() - 0.79) < 0.005
    D.check_view(ten, H, W)
    wide = D.view_records(0.0, np.radians(35.0), 0.5, H, W)
    assert D._view_w_min(wide, H, W)[0] < 0.25
    with pytest.raises(RuntimeError, match="0.25"):
        D.check_view(wide, H, W)
    # a bad matrix that serves no row is not held against the record
    v = _good()
    v["split_row"] = H
    v["ground"][:, 8] = 0.0
    D.check_view(v, H, W)
    v["split_row"] = H - 2
    with pytest.raises(RuntimeError, match="0.25"):
        D.check_view(v, H, W)


@pytest.mark.parametrize("h,w", [(9, 11), (2, 2)])
def test_restatement_never_indexes_outside_the_frame(h, w):
    """The host-side statement of the kernel's clamp: NaN, zero and negative w, infinities and huge
    entries all land inside the frame (view_one asserts its indices)."""
    f = _frame(5, h, w)
    rng = np.random.default_rng(6)
    bad = [np.nan, np.inf, -np.inf, 0.0, -1.0, 1e30, -1e30, 1e-30]
    for trial in range(200):
        v = D.identity_view(1)
        v["on"] = 1
        v["split_row"] = rng.choice([np.nan, -5.0, 3.5, 1e9])
        for name in ("far", "ground"):
            m = rng.normal(size=9) * 10.0 ** rng.integers(-3, 4)
            hit = rng.random(9) < 0.4
            m[hit] = rng.choice(bad, int(hit.sum()))
            v[name][0] = m
        out = VW.view_one(f, v[0])
        assert out.shape == f.shape and out.dtype == np.uint8
    for m8 in (0.0, -1.0, np.nan):                                  # w = 0, w < 0, w = NaN everywhere
        v = D.identity_view(1)
        v["on"] = 1
        v["far"][0, 8] = v["ground"][0, 8] = m8
        sx, sy = VW.source_coords(v[0], h, w)
        assert np.isfinite(sx).all() and sx.min() >= 0 and sx.max() <= w - 1
        assert np.isfinite(sy).all() and sy.min() >= 0 and sy.max() <= h - 1
        VW.view_one(f, v[0])


def test_mix_turns_on_its_share_inside_its_ranges():
    n = 4096
    spd = np.random.default_rng(1).random(n)
    v = D.ViewShift().draw(np.random.default_rng(8), n, spd, H, W)
    D.check_view(v, H, W)
    on = v["on"] == 1
    # binomial, p = 0.5: sigma = sqrt(n) / 2 = 32; 5 sigma
    assert abs(int(on.sum()) - n // 2) <= 160
    assert v[~on].tobytes() == D.identity_view(int((~on).sum())).tobytes()
    lat, yaw = v["lateral_m"][on], np.degrees(v["yaw_rad"][on].astype(np.float64))
    assert lat.min() >= -0.5 and lat.max() <= 0.5 and lat.max() - lat.min() > 0.9
    assert yaw.min() >= -5 - 1e-4 and yaw.max() <= 5 + 1e-4 and yaw.max() - yaw.min() > 9
    want = D.view_records(v["lateral_m"][on].astype(np.float64), v["yaw_rad"][on].astype(np.float64),
                          spd[on], H, W)
    assert np.allclose(v["steer_delta"][on], want["steer_delta"], atol=1e-6)
    q = D.ViewShift(p=0.25, lateral_m=(0.1, 0.2), yaw_deg=(1, 2)).draw(
        np.random.default_rng(8), n, spd, H, W)
    assert abs(int((q["on"] == 1).sum()) - n // 4) <= 5 * np.sqrt(n * .25 * .75)
    qon = q["on"] == 1
    assert q["lateral_m"][qon].min() >= 0.1 and (q["steer_delta"][qon] < 0).all()
    f = D.ViewShift.fixed(-0.5, 3.0).draw(np.random.default_rng(8), 50, spd[:50], H, W)
    assert (f["on"] == 1).all() and (f["lateral_m"] == -0.5).all()
    assert np.allclose(f["yaw_rad"], np.radians(3.0))
    assert (D.ViewShift(p=0.0).draw(np.random.default_rng(8), 9, spd[:9], H, W)["on"] == 0).all()
    # the stream advances by the same amount whatever is drawn
    a, b = np.random.default_rng(9), np.random.default_rng(9)
    D.ViewShift(p=0.0).draw(a, 7, spd[:7], H, W)
    D.ViewShift(p=1.0).draw(b, 7, spd[:7], H, W)
    assert a.random() == b.random()
    for bad in (dict(p=1.5), dict(lateral_m=(0.5, -0.5)), dict(yaw_deg=(1, 0))):
        with pytest.raises(ValueError):
            D.ViewShift(**bad)
    with pytest.raises(RuntimeError, match="one speed per sample"):
        D.ViewShift().draw(np.random.default_rng(0), 4, spd[:3], H, W)


class LabelsAndSpeed(LabelsOnly):
    """...and the host speeds the steering rule reads (both loaders' spellings)."""
    speed_host = speed = np.random.default_rng(12).random(len(LabelsOnly.command)).astype(np.float32)


@pytest.mark.parametrize("with_weather", [False, True])
@pytest.mark.parametrize("train", [True, False])
def test_loader_plans_with_a_view_mix(train, with_weather):
    ds = LabelsAndSpeed()
    idx = np.arange(len(ds))[::-1][:277].copy()
    bs, seed = 16, 11
    wx = (lambda: D.WeatherMix()) if with_weather else (lambda: None)

    def loader(rank=0, world=1, view=True, seed=seed):
        return D.CachedBatchLoader(ds, idx, bs, train=train, seed=seed, rank=rank, world_size=world,
                                   weather=wx(), view=D.ViewShift() if view else None)
    off, on, again = loader(view=False), loader(), loader()
    host = D.BatchLoader(ds, idx, bs, "cpu", train=train, seed=seed, weather=wx(),
                         view=D.ViewShift())
    epochs = []
    for epoch in range(3):
        if epoch == 2:
            on._plan_ahead()
        plan0, plan = off.epoch_plan(), on.epoch_plan()
        assert len(plan0) == 2 + with_weather and len(plan) == len(plan0) + 1
        order, view = plan[0], plan[-1]
        # the order, the augmentation records and the weather records of the loader without it
        assert np.array_equal(order, plan0[0])
        for a, b in zip(plan[1:-1], plan0[1:]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert view.dtype == D.VIEW_DTYPE and view.shape == order.shape
        D.check_view(view, ds.h, ds.w)
        assert 0 < (view["on"] == 1).sum() < len(view)
        # BatchLoader's stream: the same records, drawn batch by batch from the samples' speeds
        want = np.concatenate([D.ViewShift().draw(host.vrng, len(order[b:b + bs]),
                                                  ds.speed[order[b:b + bs]], ds.h, ds.w)
                               for b in range(0, len(order), bs)])
        assert view.tobytes() == want.tobytes(), epoch
        assert again.epoch_plan()[-1].tobytes() == view.tobytes()        # the same seed repeats
        epochs.append(view)
    assert epochs[0].tobytes() != epochs[1].tobytes() != epochs[2].tobytes()
    assert loader(seed=seed + 1).epoch_plan()[-1].tobytes() != epochs[0].tobytes()
    r0, r1 = loader(0, 2).epoch_plan()[-1], loader(1, 2).epoch_plan()[-1]
    assert r0.tobytes() != r1.tobytes()
    with pytest.raises(RuntimeError, match="speed_host"):
        D.CachedBatchLoader(LabelsOnly(), idx, bs, train=train, view=D.ViewShift())


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """NULL view, NULL required pointers, bad geometry and an over-wide weather call come back
    through cilrs_last_error(); nothing is dereferenced or launched, so this needs no GPU."""
    from cilrs_mi355 import _lib as L
    lib = L.lib()
    x = C.c_void_p(64)

    def augment(frames=x, params=x, weather=x, view=x, batch=4, h=88, w=200, out=x):
        return lib.cilrs_augment_view_u8(frames, params, weather, view, batch, h, w, out, None, None)

    def assemble(cache=x, index=x, params=x, weather=x, view=x, batch=4, h=88, w=200, out=x,
                 speed=None, out_speed=None):
        return lib.cilrs_batch_assemble_view(cache, 10, speed, None, None, index, params, weather,
                                             view, batch, h, w, out, None, out_speed, None, None,
                                             None)
    for fn, kwargs, text in (
            (augment, dict(view=None), "NULL argument"), (augment, dict(frames=None), "NULL argument"),
            (augment, dict(params=None), "NULL argument"), (augment, dict(out=None), "NULL argument"),
            (augment, dict(view=None, weather=None), "NULL argument"),
            (augment, dict(batch=0), "bad batch geometry"), (augment, dict(h=1), "bad batch geometry"),
            (augment, dict(weather=None, w=1), "bad batch geometry"),
            (augment, dict(w=65_409), "width 65409 above 65408"),
            (augment, dict(batch=1 << 20, h=64, w=64), "bad batch geometry"),
            (augment, dict(weather=None, batch=1 << 20, h=64, w=64), "bad batch geometry"),
            (assemble, dict(view=None), "NULL argument"), (assemble, dict(cache=None), "NULL argument"),
            (assemble, dict(view=None, weather=None), "NULL argument"),
            (assemble, dict(index=None), "NULL argument"), (assemble, dict(params=None), "NULL argument"),
            (assemble, dict(out=None), "NULL argument"),
            (assemble, dict(batch=0), "batch must be at least 1"),
            (assemble, dict(w=1), "bad batch geometry"),
            (assemble, dict(weather=None, h=1), "bad batch geometry"),
            (assemble, dict(w=65_409), "width 65409 above 65408"),
            (assemble, dict(out_speed=x), "needs its label array")):
        assert fn(**kwargs) != 0, kwargs
        assert text in lib.cilrs_last_error().decode(), (kwargs, lib.cilrs_last_error())
    with pytest.raises(RuntimeError, match="batch_assemble_view"):
        L.check(assemble(view=None))
    with pytest.raises(RuntimeError, match="augment_view"):
        L.check(augment(view=None))
