"""Weather randomisation, host side: the record layout, the float32 restatement's own properties
(identity, fog monotone in the row, rain coverage), the condition table's severity-0 identity, the
record checks, the mix, the loaders' plans with a mix, and the C entries' refusals.  No GPU needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _weather as WX
from cilrs_mi355 import data as D
from test_device_dataset_host import LabelsOnly

H, W = D.IMG_HEIGHT, D.IMG_WIDTH


def _frame(seed=0, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_record_layout_and_exports():
    import cilrs_mi355
    assert D.WEATHER_DTYPE.itemsize == 96                # cilrs_weather_params, include/cilrs_hip.h
    assert D.identity_weather(3).dtype == D.WEATHER_DTYPE
    assert D.WEATHER_CONDITIONS == ("clear", "fog", "night", "rain", "hardrain")
    for name in ("WeatherMix", "weather_condition", "weather_u8", "WEATHER_CONDITIONS"):
        assert hasattr(cilrs_mi355, name)


def test_conditions_are_the_reference_profiles():
    path = os.path.join(os.path.dirname(__file__), "golden", "weather_profiles.json")
    with open(path) as f:
        profiles = json.load(f)["weather_profiles"]
    assert set(profiles) == set(D.WEATHER_CONDITIONS)
    assert profiles["clear"]["carla_preset"] == "ClearNoon"
    assert all(isinstance(p["carla_preset"], str) and p["carla_preset"] for p in profiles.values())


def test_off_record_is_the_identity():
    f = _frame(1)
    assert np.array_equal(WX.weather_one(f, D.identity_weather(1)[0]), f)
    assert np.array_equal(WX.weather_one(f, np.zeros(1, dtype=D.WEATHER_DTYPE)[0]), f)


@pytest.mark.parametrize("name", D.WEATHER_CONDITIONS)
def test_severity_zero_is_the_identity(name):
    w = D.weather_condition(name, 0.0, 3, H, np.random.default_rng(2))
    assert w.tobytes() == D.identity_weather(3).tobytes()
    f = _frame(2)
    assert np.array_equal(WX.weather_one(f, w[0]), f)
    if name != "clear":                                  # and severity 1 is not
        w = D.weather_condition(name, 1.0, 1, H, np.random.default_rng(2))
        D.check_weather(w, H, W)
        assert not np.array_equal(WX.weather_one(f, w[0]), f)


def test_condition_table_values():
    w = D.weather_condition("hardrain", 1.0, 4, H, np.random.default_rng(3))
    assert (w["rain_len"] == 16).all() and (w["tone_on"] == 1).all() and (w["fog_on"] == 1).all()
    assert np.allclose(w["gain"], 0.65) and np.allclose(w["rain_alpha"], 0.60)
    assert (w["rain_thresh24"] == round(0.030 * (1 << 24))).all() and (w["rain_v255"] == 215).all()
    assert (np.abs(w["rain_slant_q4"]) <= 8).all() and len(set(w["rain_seed"].tolist())) == 4
    assert np.allclose(w["fog_horizon"], 0.45 * H) and np.allclose(w["fog_near"], 0.08 * H)
    w = D.weather_condition("rain", 0.5, 1, H, np.random.default_rng(3))
    assert w["rain_len"][0] == 6 and w["rain_thresh24"][0] == round(0.0075 * (1 << 24))
    w = D.weather_condition("night", 1.0, 1, H, np.random.default_rng(3))
    assert w["fog_on"][0] == 0 and w["rain_len"][0] == 0
    assert np.allclose(w["gain"][0], np.array([0.90, 0.95, 1.10]) * 0.22)
    w = D.weather_condition("fog", 0.5, 1, H, np.random.default_rng(3))
    assert w["rain_len"][0] == 0 and np.allclose(w["fog_rgb255"][0], (200, 205, 210))
    with pytest.raises(ValueError):
        D.weather_condition("snow", 0.5, 1, H, np.random.default_rng(3))
    with pytest.raises(ValueError):
        D.weather_condition("fog", 1.5, 1, H, np.random.default_rng(3))


@pytest.mark.parametrize("height", [H, 9])
def test_fog_transmission_falls_with_the_row_and_is_koschmieder_at_both_ends(height):
    beta = 1.7
    w = D.identity_weather(1)
    w["fog_on"] = 1
    w["fog_t0"], w["fog_t1"] = D.fog_transmission(beta, height)
    w["fog_horizon"], w["fog_near"] = D.FOG_HORIZON * height, D.FOG_NEAR * height
    d = WX.fog_depth(height, w["fog_horizon"][0], w["fog_near"][0])
    assert d.max() == 1 and d.min() > 0 and (np.diff(d) <= 0).all()
    t = WX.fog_transmission(w[0], height)
    # The depth does not increase with the row.  By the definition (t(1) = exp(-beta) at the
    # horizon, t(d_min) = exp(-beta * d_min) at the bottom row) the transmission then does not
    # DEcrease with it -- near ground is clearer -- and it is the fog's share 1 - t that does not
    # increase; all three are asserted.
    assert (np.diff(t) >= 0).all() and (np.diff(1 - t) <= 0).all()
    assert (t > 0).all() and (t <= 1).all() and t[-1] > t[0]
    # two float32 roundings of values below 1 around the double result: 3 * 2^-24 at most
    horizon_rows = np.arange(height) <= D.FOG_HORIZON * height
    assert np.abs(t[horizon_rows].astype(np.float64) - np.exp(-beta)).max() <= 3 * 2.0 ** -24
    d_min = D.FOG_NEAR * height / (height - 1 - D.FOG_HORIZON * height)
    # the bottom row's depth is d_min to float32 rounding; t is linear in it with slope |t1| < 1
    assert abs(float(t[-1]) - np.exp(-beta * d_min)) <= 1e-6


def test_tone_gain_one_lift_zero_is_the_identity():
    w = D.identity_weather(1)
    w["tone_on"] = 1
    f = _frame(4)
    assert np.array_equal(WX.weather_one(f, w[0]), f)
    w["gain"], w["lift255"] = (0.5, 1.0, 2.0), (0.0, -300.0, 10.0)
    out = WX.weather_one(f, w[0])
    assert np.array_equal(out[..., 0], f[..., 0] // 2) and (out[..., 1] == 0).all()
    assert np.array_equal(out[..., 2], np.minimum(f[..., 2].astype(int) * 2 + 10, 255))


RAIN_CASES = [(0.004, 6, 3), (0.016, 10, -5), (0.03, 16, 16)]


@pytest.mark.parametrize("p,length,slant", RAIN_CASES)
def test_rain_coverage_tracks_its_expectation(p, length, slant):
    w = D.identity_weather(1)
    w["rain_len"], w["rain_slant_q4"] = length, slant
    w["rain_thresh24"], w["rain_alpha"], w["rain_v255"] = int(p * (1 << 24)), 0.5, 215.0
    devs = []
    for seed in range(40):
        w["rain_seed"] = seed * 7919 + 1
        cover = (WX.rain_cover(w[0], H, W) < length).mean()
        devs.append(cover - (1 - (1 - p) ** length))
    print(p, length, slant, "mean deviation %.4f, largest single frame %.4f"
          % (np.mean(devs), np.abs(devs).max()))
    assert abs(np.mean(devs)) <= 0.01


@pytest.mark.parametrize("slant", [16, -16])
def test_rain_leaves_uncovered_pixels_alone_and_slants_both_ways(slant):
    w = D.identity_weather(1)
    w["rain_len"], w["rain_slant_q4"], w["rain_seed"] = 16, slant, 99
    w["rain_thresh24"], w["rain_alpha"], w["rain_v255"] = int(0.01 * (1 << 24)), 0.6, 215.0
    f = _frame(5, 40, 60)
    f[:4] = 215                                         # a covered pixel at the rain's own value stays
    jmin = WX.rain_cover(w[0], 40, 60)
    out = WX.weather_one(f, w[0])
    covered = jmin < 16
    assert 0.05 < covered.mean() < 0.4
    assert np.array_equal(out[~covered], f[~covered])   # bit-unchanged
    assert np.array_equal(out[:4], f[:4])
    changed = (out != f).any(-1)
    assert changed.any() and not (changed & ~covered).any()
    # a streak is a head and its tail along the slant: one column a row at +-16
    ys, xs = np.nonzero(jmin == 0)
    step = 1 if slant > 0 else -1
    k = [i for i in range(len(ys)) if ys[i] + 3 < 40 and 0 <= xs[i] + 3 * step < 60][0]
    for j in range(1, 4):
        assert jmin[ys[k] + j, xs[k] + j * step] <= j
    # heads above and beside the frame reach into it: tail positions with no head inside
    y, x = np.nonzero(covered)
    hy, hx = y - jmin[covered], x - ((jmin[covered] * slant) >> 4)
    assert ((hy < 0) | (hx < 0) | (hx >= 60)).any()


def _good():
    return D.weather_condition("hardrain", 0.8, 2, H, np.random.default_rng(6))


@pytest.mark.parametrize("field,value", [
    ("rain_len", 17), ("rain_len", -1), ("rain_slant_q4", 17), ("rain_slant_q4", -17),
    ("rain_thresh24", (1 << 24) + 1), ("rain_alpha", 1.5), ("rain_alpha", -0.1),
    ("rain_alpha", np.nan), ("rain_v255", 256.0), ("rain_v255", np.inf), ("tone_on", 2),
    ("fog_on", -1), ("gain", np.nan), ("gain", -1.0), ("lift255", np.inf), ("fog_t0", np.nan),
    ("fog_t1", -np.inf), ("fog_horizon", np.nan), ("fog_near", 0.0), ("fog_near", np.nan),
    ("fog_rgb255", 300.0), ("fog_rgb255", np.nan)])
def test_check_weather_refuses_each_bad_field(field, value):
    w = _good()
    D.check_weather(w, H, W)
    w[field][1] = value
    with pytest.raises(RuntimeError, match="weather"):
        D.check_weather(w, H, W)


def test_check_weather_refuses_dtype_and_width():
    w = _good()
    with pytest.raises(RuntimeError, match="WEATHER_DTYPE"):
        D.check_weather(w.view(np.uint8), H, W)
    with pytest.raises(RuntimeError, match="WEATHER_DTYPE"):
        D.check_weather(D.identity_params(2), H, W)
    D.check_weather(w, H, 65_408)
    with pytest.raises(RuntimeError, match="65408"):
        D.check_weather(w, H, 65_409)
    with pytest.raises(RuntimeError, match="65408"):
        D.WeatherMix().draw(np.random.default_rng(0), 1, H, 65_409)


def test_mix_hits_every_condition_within_its_severity_range():
    mix = D.WeatherMix()
    w = mix.draw(np.random.default_rng(7), 4000, H, W)
    D.check_weather(w, H, W)
    clear = (w["tone_on"] == 0)
    rainy = w["rain_len"] > 0
    fog = (w["fog_on"] == 1) & ~rainy
    night = (w["tone_on"] == 1) & (w["fog_on"] == 0)
    hard = rainy & (w["fog_rgb255"][:, 0] == 150)
    soft = rainy & (w["fog_rgb255"][:, 0] == 165)
    got = [m.mean() for m in (clear, fog, night, soft, hard)]
    assert sum(got) == pytest.approx(1.0)
    for g, want in zip(got, (.5, .125, .125, .15, .10)):   # 4000 draws: 4 sigma is 0.032 at p = .5
        assert abs(g - want) < 0.035, (got,)
    # severity in (0.2, 1.0): read back from the tone gain, 1 - dim * s
    s = (1 - w["gain"][fog, 0].astype(np.float64)) / 0.10
    assert s.min() >= 0.2 - 1e-5 and s.max() <= 1.0 + 1e-5 and s.max() - s.min() > 0.6
    s = (1 - w["gain"][hard, 0].astype(np.float64)) / 0.35
    assert s.min() >= 0.2 - 1e-5 and s.max() <= 1.0 + 1e-5
    assert (np.abs(w["rain_slant_q4"]) <= 8).all() and set(w["rain_slant_q4"][rainy]) == set(range(-8, 9))
    # fixed: every sample that condition at that severity
    f = D.WeatherMix.fixed("rain", 0.5).draw(np.random.default_rng(7), 50, H, W)
    assert (f["rain_len"] == 6).all() and np.allclose(f["gain"], 0.9)
    assert D.WeatherMix.fixed("fog", 0.0).draw(np.random.default_rng(7), 5, H, W).tobytes() \
        == D.identity_weather(5).tobytes()
    for bad in (dict(probs={"snow": 1.0}), dict(probs={"fog": 0.0}), dict(severity=(0.5, 0.2)),
                dict(severity=(0.0, 1.5))):
        with pytest.raises(ValueError):
            D.WeatherMix(**bad)


@pytest.mark.parametrize("train", [True, False])
def test_loader_plans_with_a_mix(train):
    ds = LabelsOnly()
    idx = np.arange(len(ds))[::-1][:277].copy()
    bs, seed = 16, 11

    def loader(rank=0, world=1, weather=D.WeatherMix(), seed=seed):
        return D.CachedBatchLoader(ds, idx, bs, train=train, seed=seed, rank=rank, world_size=world,
                                   weather=weather)
    off, on, again = loader(weather=None), loader(), loader()
    host = D.BatchLoader(ds, idx, bs, "cpu", train=train, seed=seed, weather=D.WeatherMix())
    epochs = []
    for epoch in range(3):
        if epoch == 2:
            on._plan_ahead()
        order0, params0 = off.epoch_plan()
        order, params, weather = on.epoch_plan()
        assert np.array_equal(order, order0) and params.tobytes() == params0.tobytes()
        assert weather.dtype == D.WEATHER_DTYPE and weather.shape == order.shape
        D.check_weather(weather, ds.h, ds.w)
        # BatchLoader's stream: the same records, drawn batch by batch
        want = np.concatenate([D.WeatherMix().draw(host.wrng, len(order[b:b + bs]), ds.h, ds.w)
                               for b in range(0, len(order), bs)])
        assert weather.tobytes() == want.tobytes(), epoch
        assert again.epoch_plan()[2].tobytes() == weather.tobytes()      # the same seed repeats
        epochs.append(weather)
    assert epochs[0].tobytes() != epochs[1].tobytes() != epochs[2].tobytes()
    assert loader(seed=seed + 1).epoch_plan()[2].tobytes() != epochs[0].tobytes()
    r0, r1 = loader(0, 2).epoch_plan()[2], loader(1, 2).epoch_plan()[2]
    assert r0.tobytes() != r1.tobytes()


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """NULL weather, NULL required pointers and bad geometry come back through
    cilrs_last_error(); nothing is dereferenced or launched, so this needs no GPU."""
    from cilrs_mi355 import _lib as L
    lib = L.lib()
    x = C.c_void_p(64)

    def augment(frames=x, params=x, weather=x, batch=4, h=88, w=200, out=x):
        return lib.cilrs_augment_weather_u8(frames, params, weather, batch, h, w, out, None, None)

    def assemble(cache=x, index=x, params=x, weather=x, batch=4, h=88, w=200, out=x, speed=None,
                 out_speed=None):
        return lib.cilrs_batch_assemble_weather(cache, 10, speed, None, None, index, params, weather,
                                                batch, h, w, out, None, out_speed, None, None, None)
    for fn, kwargs, text in (
            (augment, dict(weather=None), "NULL argument"), (augment, dict(frames=None), "NULL argument"),
            (augment, dict(params=None), "NULL argument"), (augment, dict(out=None), "NULL argument"),
            (augment, dict(batch=0), "bad batch geometry"), (augment, dict(h=1), "bad batch geometry"),
            (augment, dict(w=65_409), "width 65409 above 65408"),
            (augment, dict(batch=1 << 20, h=64, w=64), "bad batch geometry"),
            (assemble, dict(weather=None), "NULL argument"), (assemble, dict(cache=None), "NULL argument"),
            (assemble, dict(index=None), "NULL argument"), (assemble, dict(params=None), "NULL argument"),
            (assemble, dict(out=None), "NULL argument"),
            (assemble, dict(batch=0), "batch must be at least 1"),
            (assemble, dict(w=1), "bad batch geometry"),
            (assemble, dict(w=65_409), "width 65409 above 65408"),
            (assemble, dict(out_speed=x), "needs its label array")):
        assert fn(**kwargs) != 0, kwargs
        assert text in lib.cilrs_last_error().decode(), (kwargs, lib.cilrs_last_error())
    with pytest.raises(RuntimeError, match="batch_assemble_weather"):
        L.check(assemble(weather=None))
