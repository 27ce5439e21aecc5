"""oracle/augment_oracle.py against statements it does not share (tests/_augment.py): the float64
hue LUT, scipy's mirrored separable blur, float64 Box-Muller, and the reference's augmentation
policy.  The GPU tests pin the kernel to the oracle exactly; these pin the oracle, so a defect the
kernel and its float32 restatement have in common is seen here.  No GPU."""
import json
import os

import numpy as np
import pytest

import _augment as A
import augment_oracle as AO

F = np.float32


@pytest.mark.parametrize("hue", A.HUE_SWEEP)
def test_hue_shift_is_the_float64_lut_within_one_step(hue):
    H = np.arange(180, dtype=F)
    got = AO.hue_shift(H, hue).astype(np.float64)
    assert got.min() >= 0 and got.max() <= 179, (hue, got.min(), got.max())
    step = np.abs(got - A.hue_lut64(hue))
    step = np.minimum(step, 180 - step)          # one rounding of H + hue in float32
    assert step.max() <= 1, (hue, int(step.argmax()))


def test_hue_wrap_keeps_orange_red_out_of_magenta():
    """(255, 43, 0) has H = 5; hue = nextafter(-5, -6) wraps it to 179 in the LUT.  A wrap to 180
    decoded it as (255, 0, 255)."""
    hue = A.HUE_SWEEP[3]
    assert F(hue) < F(-5) and A.hue_lut64(hue)[5] == 179
    px = np.array([[[255, 43, 0]]], np.uint8)
    out = AO.augment_one(px, A.rec(hsv_on=1, hue=hue))[0, 0]
    assert out[0] == 255 and out[2] <= 1, out
    assert np.array_equal(AO.augment_one(px, A.rec(hsv_on=1, hue=-5.0))[0, 0], (255, 0, 0))


def test_hsv_round_trip_over_the_whole_cube():
    """Zero shifts only re-quantise through 8-bit HSV.  Hue is held to +-1 degree of a 60 degree
    sector (255/60 = 4.25 levels), saturation to +-0.5/255 (<= 0.5 level), the last rounding adds
    0.5: 5.25, and the outputs are integers."""
    cube = A.colour_lattice()
    out = AO.augment_one(cube, A.rec(hsv_on=1))
    assert np.abs(out.astype(np.int16) - cube.astype(np.int16)).max() <= 5


@pytest.mark.parametrize("hue,sat", [(0.0, 0.0), (-7.3, -14.2), (10.0, -20.0), (179.5, -0.5),
                                      (-360.0, -255.0), (A.HUE_SWEEP[3], 0.0), (-180.5, 0.9)])
def test_grey_stays_grey_under_hue_and_saturation(hue, sat):
    """Grey has S = 0 and the saturation LUT is trunc(clip(S + sat)): it stays 0 for every
    sat < 1, and with S = 0 no hue shows."""
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    assert np.array_equal(AO.augment_one(grey, A.rec(hsv_on=1, hue=hue, sat=sat)), grey)


def test_grey_takes_the_saturation_lut_like_any_pixel():
    """sat >= 1 lifts S = 0 to trunc(sat) as the LUT says (the 8-bit HSV of the libraries does the
    same to a grey pixel of a colour image): at H = 0 level v becomes (v, g, g) with
    g = rint(v (1 - trunc(sat) / 255))."""
    v = np.arange(256, dtype=np.float64)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    for sat in (14.2, 20.0, 255.0):
        g = np.rint(v * (1.0 - np.trunc(sat) / 255.0))
        out = AO.augment_one(grey, A.rec(hsv_on=1, sat=sat))[:, 0].astype(np.float64)
        assert np.array_equal(out[:, 0], v), sat
        assert np.abs(out[:, 1] - g).max() <= 1 and np.array_equal(out[:, 1], out[:, 2]), sat


def test_blur_is_the_mirrored_float64_gaussian():
    """float32 accumulation against float64 moves a sum across a rounding boundary rarely: one
    level, in at most 1e-4 of the elements (measured: 7 of 563,910).  The two-pixel shapes with
    five taps pin the border's period 2(n-1)."""
    from cilrs_mi355 import data as D
    rng = np.random.default_rng(11)
    bad = total = 0
    for h, w in A.EDGE_SHAPES + ((88, 200),):
        f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for k in (3, 5):
            for sigma in (0.5, 0.9, 1.1, 2.5, 3.0):
                got = AO.augment_one(f, A.rec(blur_k=k, blur_w=D.gaussian_taps(k, sigma).tolist()))
                d = np.abs(got.astype(np.float64) - A.blur64(f, k, sigma))
                assert d.max() <= 1, (h, w, k, sigma)
                bad += int((d > 0).sum())
                total += d.size
    print(f"blur: {bad} of {total} elements differ")
    assert bad <= 1e-4 * total, (bad, total)


def test_blur_border_at_two_pixels_is_periodic():
    """n = 2, radius 2: indices -2, -1, 2, 3 are 0, 1, 0, 1, so a row (a, b) blurs to
    ((w0 + 2 w2) a + 2 w1 b, 2 w1 a + (w0 + 2 w2) b)."""
    from cilrs_mi355 import data as D
    t = D.gaussian_taps(5, 1.1).astype(np.float64)
    f = np.zeros((2, 2, 3), np.uint8)
    f[:, 0] = 200
    got = AO.augment_one(f, A.rec(blur_k=5, blur_w=t.tolist()))
    want = np.rint(200.0 * np.array([t[0] + 2 * t[2], 2 * t[1]]))
    assert np.array_equal(got[0, :, 0], want) and np.array_equal(got[1, :, 2], want)
    assert np.array_equal(got, A.blur64(f, 5, 1.1))
    assert np.array_equal(AO.augment_one(f.transpose(1, 0, 2), A.rec(blur_k=5, blur_w=t.tolist())),
                          got.transpose(1, 0, 2))


@pytest.mark.parametrize("k", (3, 5))
def test_blur_keeps_a_constant_frame(k):
    from cilrs_mi355 import data as D
    for sigma in np.linspace(0.5, 3.0, 26):
        w = D.gaussian_taps(k, float(sigma)).tolist()
        for level in (0, 1, 127, 128, 254, 255):
            f = np.full((5, 6, 3), level, np.uint8)
            assert np.array_equal(AO.augment_one(f, A.rec(blur_k=k, blur_w=w)), f), (sigma, level)


def test_noise_is_float64_box_muller_on_the_same_bits():
    """float32 logf / cosf against float64 flips a rounding in at most 1e-4 of the elements
    (measured: <= 1.9e-5, one element of a sample), never by more than a level."""
    f = np.random.default_rng(12).integers(0, 256, (88, 200, 3), dtype=np.uint8)
    worst = 0.0
    for seed in A.NOISE_SEEDS:
        for sigma in A.NOISE_SIGMAS:
            got = AO.augment_one(f, A.rec(noise_std255=float(F(sigma)), noise_seed=seed))
            d = np.abs(got.astype(np.float64) - A.noisy64(f, seed, sigma))
            assert d.max() <= 1, (seed, sigma)
            worst = max(worst, float((d > 0).mean()))
            assert (d > 0).mean() <= 1e-4, (seed, sigma, float((d > 0).mean()))
    print(f"noise: largest differing share {worst:.2e}")
    a, b = A.noise64(2 ** 64 - 1, 1000), A.noise64(0, 1000)
    assert np.isfinite(a).all() and not np.array_equal(a, b)


def test_drawn_parameters_follow_the_reference_policy(golden_dir):
    from cilrs_mi355 import data as D
    with open(os.path.join(golden_dir, "augmentation_policy.json")) as fh:
        pol = json.load(fh)
    n = 20000
    p = D.draw_aug_params(np.random.default_rng(3), n)
    D.check_params(p, 88, 200)
    D.check_params(D.draw_aug_params(np.random.default_rng(3), n, 176, 400), 176, 400)

    def rate(mask, prob):
        assert abs(mask.mean() - prob) <= 4 * np.sqrt(prob * (1 - prob) / n), (mask.mean(), prob)

    def spans(x, lo, hi):
        """inside [lo, hi] (as the float32 the record stores) and within 2 % of both ends"""
        assert x.min() >= F(lo) and x.max() <= F(hi), (x.min(), x.max(), lo, hi)
        assert x.min() <= lo + 0.02 * (hi - lo) and x.max() >= hi - 0.02 * (hi - lo), (lo, hi)

    s = pol["brightness_contrast"]
    on = p["rbc_on"] == 1
    rate(on, s["p"])
    spans(p["alpha"][on], 1 - s["contrast_limit"], 1 + s["contrast_limit"])
    spans(p["beta255"][on], -255 * s["brightness_limit"], 255 * s["brightness_limit"])
    assert (p["alpha"][~on] == 1).all() and (p["beta255"][~on] == 0).all()

    s = pol["hsv"]
    on = p["hsv_on"] == 1
    rate(on, s["p"])
    for field, lim in (("hue", "hue_shift_limit"), ("sat", "sat_shift_limit"),
                       ("val", "val_shift_limit")):
        spans(p[field][on], -s[lim], s[lim])
        assert (p[field][~on] == 0).all()

    s = pol["blur"]
    on = p["blur_k"] > 1
    rate(on, s["p"])
    assert sorted(np.unique(p["blur_k"][on]).tolist()) == sorted(s["kernel_sizes"])
    assert np.isin(p["blur_k"][~on], (0, 1)).all()
    w = p["blur_w"][on].astype(np.float64)
    assert np.abs(w[:, 0] + 2 * w[:, 1] + 2 * w[:, 2] - 1).max() < 1e-6
    assert (w[p["blur_k"][on] == 3, 2] == 0).all()

    s = pol["noise"]
    on = p["noise_std255"] > 0
    rate(on, s["p"])
    spans(p["noise_std255"][on], 255 * s["std_range"][0], 255 * s["std_range"][1])

    s = pol["holes"]
    on = p["nholes"] > 0
    rate(on, s["p"])
    lo, hi = s["num_holes_range"]
    assert np.unique(p["nholes"][on]).tolist() == list(range(lo, hi + 1))
    live = np.arange(3)[None, :] < p["nholes"][:, None]
    hh = (p["hole_y1"] - p["hole_y0"])[live]
    ww = (p["hole_x1"] - p["hole_x0"])[live]
    assert np.unique(hh).tolist() == list(range(s["hole_height_range"][0],
                                                s["hole_height_range"][1] + 1))
    assert np.unique(ww).tolist() == list(range(s["hole_width_range"][0],
                                                s["hole_width_range"][1] + 1))
    assert s["fill"] == 0
    assert (p["hole_y0"][live] >= 0).all() and (p["hole_y1"][live] <= 88).all()
    assert (p["hole_x0"][live] >= 0).all() and (p["hole_x1"][live] <= 200).all()
    for field in ("hole_y0", "hole_x0", "hole_y1", "hole_x1"):
        assert (p[field][~live] == 0).all()
