"""Input pipeline for real driving data (reference notebook/notebook.ipynb:353-431,
on-disk format model/collect_data.py:545-564, 683-716, model/prepare_dataset.py:47-61).

On disk:  <data_dir>/sessionN/measurements.csv  (14 columns; this loader uses image_filename, steer,
throttle, brake, speed_normalized, command_name) and  <data_dir>/sessionN/images/frame_%08d.jpg
(200x88 JPEG).  The reference decodes and augments each frame on two CPU DataLoader workers; here
the host only parses the CSVs, draws the class-balanced sample indices and each sample's random
augmentation parameters, and decodes JPEGs on a thread pool into a pinned uint8 batch -- the
augmentation itself, /255 and Normalize run as one HIP kernel (`cilrs_augment_u8`).

`BatchLoader` decodes every frame every epoch.  When the decoded frames fit in device memory,
`DeviceDataset` decodes them once into HBM and `CachedBatchLoader` builds the same batches, bit
for bit, with one `cilrs_batch_assemble` launch each.

Both loaders take a `WeatherMix`: per-sample weather records (tone, fog, rain: the reference's
weather profiles as an image-space model) applied to the source frames inside the same launch
(`cilrs_augment_weather_u8`, `cilrs_batch_assemble_weather`).  Without one nothing differs.

Both also take a `ViewShift`: per-sample viewpoint records (a camera moved sideways and yawed,
as two homographies split at the horizon) applied in front of the weather in the same launch
(`cilrs_augment_view_u8`, `cilrs_batch_assemble_view`), with the steer label corrected by a
pure-pursuit rule.  Without one nothing differs either.
"""
from __future__ import annotations

import csv
import ctypes as C
import os
import queue
import threading

import numpy as np
import torch

from . import _lib as L

COMMAND_MAP = {"LANEFOLLOW": 0, "LEFT": 1, "RIGHT": 2, "STRAIGHT": 3}     # notebook.ipynb:358
IMG_HEIGHT, IMG_WIDTH = 88, 200

# numpy mirror of `cilrs_aug_params` (include/cilrs_hip.h), 112 bytes
AUG_DTYPE = np.dtype([
    ("noise_seed", np.uint64), ("rbc_on", np.int32), ("alpha", np.float32),
    ("beta255", np.float32), ("hsv_on", np.int32), ("hue", np.float32), ("sat", np.float32),
    ("val", np.float32), ("blur_k", np.int32), ("blur_w", np.float32, 3),
    ("noise_std255", np.float32), ("nholes", np.int32), ("hole_y0", np.int32, 3),
    ("hole_x0", np.int32, 3), ("hole_y1", np.int32, 3), ("hole_x1", np.int32, 3),
    ("reserved", np.int32)], align=True)
assert AUG_DTYPE.itemsize == 112


def identity_params(batch: int) -> np.ndarray:
    """Every augmentation off (validation: only /255 + Normalize)."""
    p = np.zeros(batch, dtype=AUG_DTYPE)
    p["alpha"] = 1.0
    return p


def gaussian_taps(ksize: int, sigma: float) -> np.ndarray:
    """cv2.getGaussianKernel(ksize, sigma) as (centre, +-1, +-2) float32 weights."""
    r = ksize // 2
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(x * x) / (2.0 * sigma * sigma))
    w /= w.sum()
    out = np.zeros(3, dtype=np.float32)
    out[:r + 1] = w[r:].astype(np.float32)
    return out


def draw_aug_params(rng: np.random.Generator, batch: int, height: int = IMG_HEIGHT,
                    width: int = IMG_WIDTH) -> np.ndarray:
    """Per-sample parameters of the reference's train_augmentation (notebook.ipynb:387-394):
    RandomBrightnessContrast(0.2, 0.2, p=.5), HueSaturationValue(10, 20, 15, p=.3),
    GaussianBlur(blur_limit=(3,5), p=.2), GaussNoise(std_range=(.02,.06), p=.3),
    CoarseDropout(1-3 holes, h 4-10, w 8-20, fill 0, p=.2)."""
    p = identity_params(batch)
    on = rng.random((5, batch))
    m = on[0] < 0.5
    p["rbc_on"] = m
    p["alpha"] = np.where(m, 1.0 + rng.uniform(-0.2, 0.2, batch), 1.0)
    p["beta255"] = np.where(m, rng.uniform(-0.2, 0.2, batch) * 255.0, 0.0)
    m = on[1] < 0.3
    p["hsv_on"] = m
    p["hue"] = np.where(m, rng.uniform(-10, 10, batch), 0.0)
    p["sat"] = np.where(m, rng.uniform(-20, 20, batch), 0.0)
    p["val"] = np.where(m, rng.uniform(-15, 15, batch), 0.0)
    m = on[2] < 0.2
    ks = rng.choice((3, 5), batch)
    sig = rng.uniform(0.5, 3.0, batch)
    for i in np.nonzero(m)[0]:
        p["blur_k"][i] = ks[i]
        p["blur_w"][i] = gaussian_taps(int(ks[i]), float(sig[i]))
    m = on[3] < 0.3
    p["noise_std255"] = np.where(m, rng.uniform(0.02, 0.06, batch) * 255.0, 0.0)
    p["noise_seed"] = np.where(m, rng.integers(0, 1 << 63, batch, dtype=np.uint64), np.uint64(0))
    m = on[4] < 0.2
    nh = rng.integers(1, 4, batch)
    hh = rng.integers(4, 11, (batch, 3))
    ww = rng.integers(8, 21, (batch, 3))
    y0 = (rng.random((batch, 3)) * (height - hh + 1)).astype(np.int64)
    x0 = (rng.random((batch, 3)) * (width - ww + 1)).astype(np.int64)
    live = m[:, None] & (np.arange(3)[None, :] < nh[:, None])
    p["nholes"] = np.where(m, nh, 0)
    p["hole_y0"] = np.where(live, y0, 0)
    p["hole_x0"] = np.where(live, x0, 0)
    p["hole_y1"] = np.where(live, y0 + hh, 0)
    p["hole_x1"] = np.where(live, x0 + ww, 0)
    return p


def check_params(p: np.ndarray, height: int, width: int):
    if p.dtype != AUG_DTYPE:
        raise RuntimeError("augmentation parameters must use data.AUG_DTYPE")
    if not np.isin(p["blur_k"], (0, 1, 3, 5)).all():
        raise RuntimeError("blur_k must be 0, 1, 3 or 5")
    if (p["nholes"] < 0).any() or (p["nholes"] > 3).any():
        raise RuntimeError("nholes must be 0..3")
    if (p["hole_y1"] > height).any() or (p["hole_x1"] > width).any() or \
            (p["hole_y0"] < 0).any() or (p["hole_x0"] < 0).any():
        raise RuntimeError("dropout hole outside the frame")


# ---- weather: tone, fog and rain in front of the augmentation -----------------------------------
# numpy mirror of `cilrs_weather_params` (include/cilrs_hip.h, where the stages are defined), 96 bytes
WEATHER_DTYPE = np.dtype([
    ("rain_seed", np.uint64), ("tone_on", np.int32), ("gain", np.float32, 3),
    ("lift255", np.float32, 3), ("fog_on", np.int32), ("fog_t0", np.float32),
    ("fog_t1", np.float32), ("fog_horizon", np.float32), ("fog_near", np.float32),
    ("fog_rgb255", np.float32, 3), ("rain_len", np.int32), ("rain_slant_q4", np.int32),
    ("rain_thresh24", np.uint32), ("rain_alpha", np.float32), ("rain_v255", np.float32),
    ("reserved", np.int32, 2)], align=True)
assert WEATHER_DTYPE.itemsize == 96

# the reference's five weather profiles (configs/weather_config.json), clear first
WEATHER_CONDITIONS = ("clear", "fog", "night", "rain", "hardrain")
WEATHER_MAX_WIDTH = 65536 - 128       # streak heads are hashed from (row + 64, column + 64) in 16 bits each
WEATHER_MAX_RAIN_LEN = 16
WEATHER_STREAM = 0x57454154           # "WEAT": third key of the loaders' weather record stream
FOG_HORIZON, FOG_NEAR = 0.45, 0.08    # of the frame height: horizon row, nearest ground depth

# Initial constants, linear in severity s in [0, 1]; CARLA's renderer is not available here, so the
# look is parity-unpinned.  tint * (1 - dim * s) = tone gain; beta * s = fog extinction at depth 1;
# p0 + p1 * s = streak-head probability; round(len0 + len1 * s) = streak length; a0 + a1 * s = alpha.
_CONDITION_TABLE = {
    "fog": dict(dim=0.10, tint=(1.0, 1.0, 1.0), beta=3.0, air=(200.0, 205.0, 210.0)),
    "night": dict(dim=0.78, tint=(0.90, 0.95, 1.10), beta=0.0, air=(0.0, 0.0, 0.0)),
    "rain": dict(dim=0.20, tint=(1.0, 1.0, 1.0), beta=0.8, air=(165.0, 170.0, 175.0),
                 p=(0.003, 0.009), length=(4.0, 4.0), alpha=(0.30, 0.15), v=215.0),
    "hardrain": dict(dim=0.35, tint=(1.0, 1.0, 1.0), beta=1.6, air=(150.0, 155.0, 160.0),
                     p=(0.008, 0.022), length=(6.0, 10.0), alpha=(0.35, 0.25), v=215.0),
}


def identity_weather(batch: int) -> np.ndarray:
    """Every weather stage off: the records under which the weather kernels give what the plain
    ones give."""
    p = np.zeros(batch, dtype=WEATHER_DTYPE)
    p["gain"] = 1.0
    return p


def fog_transmission(beta: float, height: int):
    """(t0, t1) of t(d) = t0 + t1 * d with t(1) = exp(-beta) and t(d_min) = exp(-beta * d_min),
    d_min = near / (H - 1 - horizon) the depth of the bottom row: Koschmieder's law interpolated
    linearly in depth between the far and the near end.  Computed in double."""
    horizon, near = FOG_HORIZON * height, FOG_NEAR * height
    span = height - 1 - horizon
    d_min = near / span if span > near else 1.0
    far = float(np.exp(-beta))
    if d_min >= 1.0:
        return far, 0.0
    t1 = (far - float(np.exp(-beta * d_min))) / (1.0 - d_min)
    return far - t1, t1


def _condition_records(names, severity, height, seeds, slants) -> np.ndarray:
    """One record per sample from its condition name, severity, rain seed and slant."""
    n = len(names)
    p = identity_weather(n)
    for i in range(n):
        name, s = names[i], float(severity[i])
        if name not in WEATHER_CONDITIONS:
            raise ValueError(f"unknown weather condition {name!r}; one of {WEATHER_CONDITIONS}")
        if not (0.0 <= s <= 1.0):
            raise ValueError(f"weather severity {s} outside [0, 1]")
        if name == "clear" or s == 0.0:
            continue
        c, r = _CONDITION_TABLE[name], p[i:i + 1]
        r["tone_on"] = 1
        r["gain"] = [(1.0 - c["dim"] * s) * t for t in c["tint"]]
        beta = c["beta"] * s
        if beta > 0.0:
            r["fog_on"] = 1
            r["fog_t0"], r["fog_t1"] = fog_transmission(beta, height)
            r["fog_horizon"], r["fog_near"] = FOG_HORIZON * height, FOG_NEAR * height
            r["fog_rgb255"] = c["air"]
        if "p" in c:
            r["rain_len"] = int(np.floor(c["length"][0] + c["length"][1] * s + 0.5))
            r["rain_thresh24"] = int(round((c["p"][0] + c["p"][1] * s) * (1 << 24)))
            r["rain_alpha"] = c["alpha"][0] + c["alpha"][1] * s
            r["rain_v255"] = c["v"]
            r["rain_slant_q4"] = int(slants[i])
            r["rain_seed"] = seeds[i]
    return p


def _draw_rain_keys(rng: np.random.Generator, n: int):
    """Per-sample rain seed and slant (uniform integer in [-8, 8] columns per 16 rows); drawn for
    every sample, rainy or not, so the stream advances the same way under any mix."""
    return rng.integers(0, 1 << 63, n, dtype=np.uint64), rng.integers(-8, 9, n)


def weather_condition(name: str, severity: float, n: int, height: int = IMG_HEIGHT,
                      rng: np.random.Generator = None) -> np.ndarray:
    """n records of condition `name` (one of WEATHER_CONDITIONS) at `severity` in [0, 1]; severity
    0 is the identity for every name.  The rain seed and slant are drawn per sample from `rng`."""
    rng = np.random.default_rng(0) if rng is None else rng
    seeds, slants = _draw_rain_keys(rng, n)
    return _condition_records([name] * n, np.full(n, float(severity)), height, seeds, slants)


class WeatherMix:
    """What weather a loader draws: condition `name` with probability probs[name], its severity
    uniform in `severity` = (low, high)."""

    DEFAULT_PROBS = {"clear": .5, "fog": .125, "night": .125, "rain": .15, "hardrain": .10}

    def __init__(self, probs: dict = None, severity=(0.2, 1.0)):
        probs = dict(self.DEFAULT_PROBS if probs is None else probs)
        for k, v in probs.items():
            if k not in WEATHER_CONDITIONS:
                raise ValueError(f"unknown weather condition {k!r}; one of {WEATHER_CONDITIONS}")
            if not (v >= 0.0):
                raise ValueError(f"probability of {k!r} must be non-negative")
        total = float(sum(probs.values()))
        if not (total > 0.0):
            raise ValueError("WeatherMix: the probabilities sum to zero")
        lo, hi = float(severity[0]), float(severity[1])
        if not (0.0 <= lo <= hi <= 1.0):
            raise ValueError("WeatherMix: severity must be (low, high) with 0 <= low <= high <= 1")
        self.names = tuple(k for k in WEATHER_CONDITIONS if probs.get(k, 0.0) > 0.0)
        self.cum = np.cumsum([probs[k] / total for k in self.names])
        self.cum[-1] = 1.0
        self.severity = (lo, hi)

    @classmethod
    def fixed(cls, name: str, severity: float):
        """Every sample gets condition `name` at `severity`."""
        return cls({name: 1.0}, (severity, severity))

    def draw(self, rng: np.random.Generator, n: int, height: int = IMG_HEIGHT,
             width: int = IMG_WIDTH) -> np.ndarray:
        """n records; advances `rng` by the same amount whatever is drawn."""
        if width > WEATHER_MAX_WIDTH:
            raise RuntimeError(f"weather: width {width} above {WEATHER_MAX_WIDTH}")
        pick = np.searchsorted(self.cum, rng.random(n), side="right")
        pick = np.minimum(pick, len(self.names) - 1)
        sev = rng.uniform(self.severity[0], self.severity[1], n)
        seeds, slants = _draw_rain_keys(rng, n)
        return _condition_records([self.names[k] for k in pick], sev, height, seeds, slants)


def check_weather(p: np.ndarray, height: int, width: int):
    if not isinstance(p, np.ndarray) or p.dtype != WEATHER_DTYPE:
        raise RuntimeError("weather records must use data.WEATHER_DTYPE")
    if width > WEATHER_MAX_WIDTH:
        raise RuntimeError(f"weather: width {width} above {WEATHER_MAX_WIDTH}")
    for k in ("gain", "lift255", "fog_t0", "fog_t1", "fog_horizon", "fog_near", "fog_rgb255",
              "rain_alpha", "rain_v255"):
        if not np.isfinite(p[k]).all():
            raise RuntimeError(f"weather: {k} must be finite")
    if not np.isin(p["tone_on"], (0, 1)).all() or not np.isin(p["fog_on"], (0, 1)).all():
        raise RuntimeError("weather: tone_on and fog_on must be 0 or 1")
    if (p["gain"] < 0).any():
        raise RuntimeError("weather: gain must be non-negative")
    fog = p["fog_on"] == 1
    if (p["fog_near"][fog] <= 0).any():
        raise RuntimeError("weather: fog_near must be positive where fog is on")
    if (p["fog_rgb255"] < 0).any() or (p["fog_rgb255"] > 255).any():
        raise RuntimeError("weather: fog_rgb255 must lie in [0, 255]")
    if (p["rain_len"] < 0).any() or (p["rain_len"] > WEATHER_MAX_RAIN_LEN).any():
        raise RuntimeError(f"weather: rain_len must be 0..{WEATHER_MAX_RAIN_LEN}")
    if (np.abs(p["rain_slant_q4"].astype(np.int64)) > 16).any():
        raise RuntimeError("weather: rain_slant_q4 must lie in [-16, 16]")
    if (p["rain_thresh24"] > (1 << 24)).any():
        raise RuntimeError("weather: rain_thresh24 must be at most 2^24")
    if (p["rain_alpha"] < 0).any() or (p["rain_alpha"] > 1).any():
        raise RuntimeError("weather: rain_alpha must lie in [0, 1]")
    if (p["rain_v255"] < 0).any() or (p["rain_v255"] > 255).any():
        raise RuntimeError("weather: rain_v255 must lie in [0, 255]")


# ---- viewpoint: lateral offset and yaw in front of the weather -----------------------------------
# numpy mirror of `cilrs_view_params` (include/cilrs_hip.h, where the warp is defined), 96 bytes
VIEW_DTYPE = np.dtype([
    ("on", np.int32), ("split_row", np.float32), ("far", np.float32, 9),
    ("ground", np.float32, 9), ("steer_delta", np.float32), ("lateral_m", np.float32),
    ("yaw_rad", np.float32), ("reserved", np.int32)], align=True)
assert VIEW_DTYPE.itemsize == 96

VIEW_STREAM = 0x56494557              # "VIEW": third key of the loaders' viewpoint record stream
VIEW_MIN_W = 0.25                     # smallest homogeneous w a record may reach inside the frame
SPEED_NORM_KMH = 40.0                 # speed_normalized = km/h / 40 (model/collect_data.py)


class CameraModel:
    """The reference's camera (model/collect_data.py Config, model/prepare_dataset.py): 800x600 at
    100 degrees horizontal field of view, no pitch, `height_m` above a flat road, resized to the
    training frame without cropping -- so the two focal lengths differ."""

    def __init__(self, width0: int = 800, height0: int = 600, fov_deg: float = 100.0,
                 height_m: float = 1.4):
        self.width0, self.height0 = int(width0), int(height0)
        self.fov_deg, self.height_m = float(fov_deg), float(height_m)
        if not (0.0 < self.fov_deg < 180.0) or not (self.height_m > 0.0):
            raise ValueError("CameraModel: fov_deg in (0, 180) and height_m > 0")
        self.f0 = 0.5 * self.width0 / np.tan(np.radians(0.5 * self.fov_deg))

    def intrinsics(self, height: int, width: int):
        """(fx, fy, cx, cy) of the H x W training frame, float64."""
        return (self.f0 * width / self.width0, self.f0 * height / self.height0,
                0.5 * (width - 1), 0.5 * (height - 1))


def identity_view(n: int) -> np.ndarray:
    """n records that are off (and hold the identity map): under them the view entry points give
    what the weather / plain ones give."""
    p = np.zeros(n, dtype=VIEW_DTYPE)
    p["far"] = p["ground"] = np.eye(3, dtype=np.float32).reshape(9)
    return p


def steer_correction(lateral_m, yaw_rad, speed_norm, lookahead_s: float = 1.0,
                     min_lookahead_m: float = 4.0, wheelbase_m: float = 2.875,
                     max_steer_deg: float = 70.0) -> np.ndarray:
    """Pure pursuit towards the expert's path from the displaced pose, float64 [n]: the point the
    expert reaches after the look-ahead L = max(lookahead_s * v, min_lookahead_m) lies
    yt = -t cos(psi) - L sin(psi) to the right of the virtual camera's axis, and the bicycle model
    steers atan(wheelbase * 2 yt / L^2), as a share of the largest wheel angle.  v is the speed in
    m/s (speed_norm * 40 km/h).  The defaults are the reference's Tesla Model 3 in CARLA and a
    one-second look-ahead: stated assumptions, not measured ones."""
    t = np.asarray(lateral_m, dtype=np.float64)
    psi = np.asarray(yaw_rad, dtype=np.float64)
    v = np.asarray(speed_norm, dtype=np.float64) * SPEED_NORM_KMH / 3.6
    t, psi, v = np.broadcast_arrays(t, psi, v)
    look = np.maximum(lookahead_s * v, min_lookahead_m)
    yt = 0.0 - t * np.cos(psi) - look * np.sin(psi)              # (0, 0) gives +0.0
    return np.arctan(wheelbase_m * 2.0 * yt / (look * look)) / np.radians(max_steer_deg)


def view_records(lateral_m, yaw_rad, speed_norm, height: int = IMG_HEIGHT,
                 width: int = IMG_WIDTH, camera: CameraModel = None, **steer_kw) -> np.ndarray:
    """One record (on = 1) per sample for a virtual camera moved `lateral_m` to the right and yawed
    `yaw_rad` to the right of the recording one: X' = R (X - T), T = (t, 0, 0), camera x right,
    y down, z forward.  Points at infinity map by K R K^-1 (`far`), points of the flat road
    n^T X = h, n = (0, 1, 0), by K R (I - T n^T / h) K^-1 (`ground`); both are built in float64,
    inverted in closed form ((I - T n^T / h)^-1 = I + T n^T / h because n^T T = 0), scaled so that
    w = 1 at the principal point and cast to float32.  The horizon row (H-1)/2 stays put under
    this motion and the two maps agree on it: it is the split row.  A zero motion gives the
    identity map exactly.  steer_kw: the arguments of `steer_correction`."""
    camera = CameraModel() if camera is None else camera
    t, psi, spd = np.broadcast_arrays(np.atleast_1d(np.asarray(lateral_m, dtype=np.float64)),
                                      np.atleast_1d(np.asarray(yaw_rad, dtype=np.float64)),
                                      np.atleast_1d(np.asarray(speed_norm, dtype=np.float64)))
    n = len(t)
    fx, fy, cx, cy = camera.intrinsics(height, width)
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    Kinv = np.array([[1.0 / fx, 0.0, -cx / fx], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]])
    centre = np.array([cx, cy, 1.0])
    p = identity_view(n)
    p["on"] = 1
    p["split_row"] = cy
    p["lateral_m"], p["yaw_rad"] = t, psi
    p["steer_delta"] = steer_correction(t, psi, spd, **steer_kw)
    eye = np.eye(3)
    c, s = np.cos(psi), np.sin(psi)
    Rt = np.zeros((n, 3, 3))                                                # R^T: R yaws right
    Rt[:, 0, 0], Rt[:, 0, 2], Rt[:, 1, 1], Rt[:, 2, 0], Rt[:, 2, 2] = c, s, 1.0, -s, c
    shear = np.broadcast_to(eye, (n, 3, 3)).copy()                          # I + T n^T / h
    shear[:, 0, 1] = t / camera.height_m
    for name, B in (("far", Rt), ("ground", shear @ Rt)):
        M = K @ B @ Kinv
        M = M / (M[:, 2, :] @ centre)[:, None, None]
        M[(B == eye).all(axis=(1, 2))] = eye                                # K I K^-1, exactly
        p[name] = M.reshape(n, 9)
    return p


def _view_w_min(p: np.ndarray, height: int, width: int) -> np.ndarray:
    """Smallest w of each record over the rows its two matrices serve, float64 [n]; w is linear in
    (x, y), so the corners of the two row bands suffice."""
    split = p["split_row"].astype(np.float64)
    last_far = np.clip(np.floor(split), -1, height - 1)          # far: rows 0 .. last_far
    wmin = np.full(len(p), np.inf)
    for name, y_lo, y_hi in (("far", np.zeros(len(p)), last_far),
                             ("ground", last_far + 1, np.full(len(p), height - 1.0))):
        m = p[name].astype(np.float64)
        served = y_hi >= y_lo
        for y in (y_lo, y_hi):
            for x in (0.0, width - 1.0):
                w = m[:, 6] * x + m[:, 7] * y + m[:, 8]
                wmin = np.where(served, np.minimum(wmin, w), wmin)
    return wmin


def check_view(p: np.ndarray, height: int, width: int):
    if not isinstance(p, np.ndarray) or p.dtype != VIEW_DTYPE:
        raise RuntimeError("view records must use data.VIEW_DTYPE")
    for k in ("split_row", "far", "ground", "steer_delta", "lateral_m", "yaw_rad"):
        if not np.isfinite(p[k]).all():
            raise RuntimeError(f"view: {k} must be finite")
    if not np.isin(p["on"], (0, 1)).all():
        raise RuntimeError("view: on must be 0 or 1")
    if (p["split_row"] < -1).any() or (p["split_row"] > height).any():
        raise RuntimeError(f"view: split_row must lie in [-1, {height}]")
    if (np.abs(p["steer_delta"]) > 2).any():
        raise RuntimeError("view: |steer_delta| must be at most 2")
    if len(p) and (_view_w_min(p, height, width) < VIEW_MIN_W).any():
        raise RuntimeError(f"view: w falls below {VIEW_MIN_W} inside the frame (the motion is too "
                           "large for this camera)")


class ViewShift:
    """What viewpoint a loader draws: with probability p a sample is seen from a camera moved
    uniformly in `lateral_m` = (low, high) metres and yawed uniformly in `yaw_deg` = (low, high)
    degrees, and its steer label is corrected by `steer_correction`; the other samples get an off
    record.  steer_kw: the arguments of `steer_correction`."""

    def __init__(self, p: float = 0.5, lateral_m=(-0.5, 0.5), yaw_deg=(-5.0, 5.0),
                 camera: CameraModel = None, **steer_kw):
        if not (0.0 <= p <= 1.0):
            raise ValueError("ViewShift: p must lie in [0, 1]")
        self.p = float(p)
        self.lateral_m = (float(lateral_m[0]), float(lateral_m[1]))
        self.yaw_deg = (float(yaw_deg[0]), float(yaw_deg[1]))
        if self.lateral_m[0] > self.lateral_m[1] or self.yaw_deg[0] > self.yaw_deg[1]:
            raise ValueError("ViewShift: ranges are (low, high) with low <= high")
        self.camera = CameraModel() if camera is None else camera
        steer_correction(0.0, 0.0, 0.0, **steer_kw)            # refuses an unknown argument now
        self.steer_kw = steer_kw

    @classmethod
    def fixed(cls, lateral_m: float, yaw_deg: float, **kw):
        """Every sample from the one viewpoint (lateral_m, yaw_deg)."""
        return cls(1.0, (lateral_m, lateral_m), (yaw_deg, yaw_deg), **kw)

    def draw(self, rng: np.random.Generator, n: int, speed_norm, height: int = IMG_HEIGHT,
             width: int = IMG_WIDTH) -> np.ndarray:
        """n records for samples of normalised speed `speed_norm` [n]; advances `rng` by the same
        amount whatever is drawn."""
        speed_norm = np.asarray(speed_norm, dtype=np.float64).reshape(-1)
        if speed_norm.shape != (n,):
            raise RuntimeError("ViewShift.draw: one speed per sample")
        on = rng.random(n) < self.p
        lat = rng.uniform(self.lateral_m[0], self.lateral_m[1], n)
        yaw = np.radians(rng.uniform(self.yaw_deg[0], self.yaw_deg[1], n))
        rec = identity_view(n)
        if on.any():
            rec[on] = view_records(lat[on], yaw[on], speed_norm[on], height, width, self.camera,
                                   **self.steer_kw)
        return rec


def correct_steer(targets: np.ndarray, view: np.ndarray) -> np.ndarray:
    """targets float32 [n, 3] with the steer column corrected as `cilrs_batch_assemble_view` does:
    one float32 add and a clip to [-1, 1] where the record is on, a copy where it is off."""
    out = np.array(targets, dtype=np.float32, copy=True)
    on = view["on"] != 0
    moved = out[on, 0] + view["steer_delta"][on]
    out[on, 0] = np.fmin(np.fmax(moved, np.float32(-1)), np.float32(1))
    return out


def _records_to_device(rec: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(
        len(rec), rec.dtype.itemsize)).to(device, non_blocking=False)


def augment_u8(frames_u8: torch.Tensor, params: np.ndarray, want_u8: bool = False,
               params_dev: torch.Tensor = None, weather: np.ndarray = None,
               weather_dev: torch.Tensor = None, view: np.ndarray = None,
               view_dev: torch.Tensor = None):
    """frames uint8 [B,H,W,3] on the device + per-sample parameters -> normalised image as the
    logical NCHW float tensor `CILRS.forward` takes (a permuted view of the NHWC result, like the
    reference's permute at notebook.ipynb:413) [, augmented uint8 frames].

    weather: one WEATHER_DTYPE record per frame, applied to the source pixels in the same launch
    (`cilrs_augment_weather_u8`); None is the plain `cilrs_augment_u8`.  weather_dev: the same
    records already on the device (uint8 [B, 96]), like params_dev.

    view / view_dev: one VIEW_DTYPE record per frame, likewise; the frames are seen from the
    records' viewpoints before the weather and everything else (`cilrs_augment_view_u8`, with or
    without weather).  The label correction is the caller's (`correct_steer`)."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.size(3) != 3 \
            or frames_u8.device.type != "cuda":
        raise RuntimeError("augment_u8: frames must be uint8 [B,H,W,3] on the GPU (no CPU fallback)")
    b, h, w = frames_u8.size(0), frames_u8.size(1), frames_u8.size(2)
    if params.shape != (b,):
        raise RuntimeError("augment_u8: one parameter record per frame")
    check_params(params, h, w)
    if weather is None and weather_dev is not None:
        raise RuntimeError("augment_u8: weather_dev needs the host records in `weather` too")
    if weather is not None:
        if weather.shape != (b,):
            raise RuntimeError("augment_u8: one weather record per frame")
        check_weather(weather, h, w)
    if view is None and view_dev is not None:
        raise RuntimeError("augment_u8: view_dev needs the host records in `view` too")
    if view is not None:
        if not isinstance(view, np.ndarray) or view.shape != (b,):
            raise RuntimeError("augment_u8: one view record per frame")
        check_view(view, h, w)
    frames_u8 = frames_u8.contiguous()
    # params_dev: the same records already on the device (uint8 [B, 112]; the loader uploads them
    # from pinned memory on its copy stream).  Without it they go up from pageable memory, which
    # makes the host wait for everything queued on this stream -- fine for one-off calls, a full
    # host-device synchronisation per step inside a training loop.
    if params_dev is not None:
        if params_dev.dtype != torch.uint8 or tuple(params_dev.shape) != (b, AUG_DTYPE.itemsize) \
                or params_dev.device != frames_u8.device:
            raise RuntimeError("augment_u8: params_dev must be uint8 [B, %d] on the frames' device"
                               % AUG_DTYPE.itemsize)
        pdev = params_dev.contiguous()
    else:
        pdev = torch.from_numpy(params.view(np.uint8).reshape(b, AUG_DTYPE.itemsize)).to(
            frames_u8.device, non_blocking=False)
    wdev = None
    if weather_dev is not None:
        if weather_dev.dtype != torch.uint8 \
                or tuple(weather_dev.shape) != (b, WEATHER_DTYPE.itemsize) \
                or weather_dev.device != frames_u8.device:
            raise RuntimeError("augment_u8: weather_dev must be uint8 [B, %d] on the frames' device"
                               % WEATHER_DTYPE.itemsize)
        wdev = weather_dev.contiguous()
    elif weather is not None:
        wdev = _records_to_device(weather, frames_u8.device)
    vdev = None
    if view_dev is not None:
        if view_dev.dtype != torch.uint8 or tuple(view_dev.shape) != (b, VIEW_DTYPE.itemsize) \
                or view_dev.device != frames_u8.device:
            raise RuntimeError("augment_u8: view_dev must be uint8 [B, %d] on the frames' device"
                               % VIEW_DTYPE.itemsize)
        vdev = view_dev.contiguous()
    elif view is not None:
        vdev = _records_to_device(view, frames_u8.device)
    out = torch.empty(b, h, w, 3, dtype=torch.float32, device=frames_u8.device)
    out8 = torch.empty_like(frames_u8) if want_u8 else None
    stream = torch.cuda.current_stream(frames_u8.device).cuda_stream
    if vdev is not None:
        L.check(L.lib().cilrs_augment_view_u8(L.ptr(frames_u8), L.ptr(pdev), L.ptr(wdev),
                                              L.ptr(vdev), b, h, w, L.ptr(out), L.ptr(out8),
                                              C.c_void_p(stream)))
    elif wdev is None:
        L.check(L.lib().cilrs_augment_u8(L.ptr(frames_u8), L.ptr(pdev), b, h, w, L.ptr(out),
                                         L.ptr(out8), C.c_void_p(stream)))
    else:
        L.check(L.lib().cilrs_augment_weather_u8(L.ptr(frames_u8), L.ptr(pdev), L.ptr(wdev), b, h,
                                                 w, L.ptr(out), L.ptr(out8), C.c_void_p(stream)))
    img = out.permute(0, 3, 1, 2)
    return (img, out8) if want_u8 else img


def weather_u8(frames_u8: torch.Tensor, weather: np.ndarray) -> torch.Tensor:
    """frames uint8 [B,H,W,3] on the device + one WEATHER_DTYPE record per frame -> the frames
    under that weather, uint8 [B,H,W,3]: what the model is shown, to look at or to hand to a
    `Predictor`.  One `cilrs_augment_weather_u8` launch with every augmentation off and only the
    byte output asked for."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.size(3) != 3 \
            or frames_u8.device.type != "cuda":
        raise RuntimeError("weather_u8: frames must be uint8 [B,H,W,3] on the GPU (no CPU fallback)")
    b, h, w = frames_u8.size(0), frames_u8.size(1), frames_u8.size(2)
    if not isinstance(weather, np.ndarray) or weather.shape != (b,):
        raise RuntimeError("weather_u8: one weather record per frame")
    check_weather(weather, h, w)
    frames_u8 = frames_u8.contiguous()
    pdev = _records_to_device(identity_params(b), frames_u8.device)
    wdev = _records_to_device(weather, frames_u8.device)
    out8 = torch.empty_like(frames_u8)
    stream = torch.cuda.current_stream(frames_u8.device).cuda_stream
    L.check(L.lib().cilrs_augment_weather_u8(L.ptr(frames_u8), L.ptr(pdev), L.ptr(wdev), b, h, w,
                                             None, L.ptr(out8), C.c_void_p(stream)))
    return out8


def view_u8(frames_u8: torch.Tensor, view: np.ndarray) -> torch.Tensor:
    """frames uint8 [B,H,W,3] on the device + one VIEW_DTYPE record per frame -> the frames from
    those viewpoints, uint8 [B,H,W,3]: what the model is shown.  One `cilrs_augment_view_u8`
    launch with no weather, every augmentation off and only the byte output asked for."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.size(3) != 3 \
            or frames_u8.device.type != "cuda":
        raise RuntimeError("view_u8: frames must be uint8 [B,H,W,3] on the GPU (no CPU fallback)")
    b, h, w = frames_u8.size(0), frames_u8.size(1), frames_u8.size(2)
    if not isinstance(view, np.ndarray) or view.shape != (b,):
        raise RuntimeError("view_u8: one view record per frame")
    check_view(view, h, w)
    frames_u8 = frames_u8.contiguous()
    pdev = _records_to_device(identity_params(b), frames_u8.device)
    vdev = _records_to_device(view, frames_u8.device)
    out8 = torch.empty_like(frames_u8)
    stream = torch.cuda.current_stream(frames_u8.device).cuda_stream
    L.check(L.lib().cilrs_augment_view_u8(L.ptr(frames_u8), L.ptr(pdev), None, L.ptr(vdev), b, h,
                                          w, None, L.ptr(out8), C.c_void_p(stream)))
    return out8


# ---- dataset on disk -------------------------------------------------------------------------
class Sessions:
    """All `sessionN/measurements.csv` under data_dir, concatenated (notebook.ipynb:360-372)."""

    def __init__(self, data_dir: str):
        names = sorted(d for d in os.listdir(data_dir)
                       if os.path.isdir(os.path.join(data_dir, d)) and "session" in d)
        if not names:
            raise RuntimeError(f"no session directories under {data_dir}")
        paths, cols = [], {k: [] for k in ("steer", "throttle", "brake", "speed_normalized")}
        cmds = []
        for s in names:
            with open(os.path.join(data_dir, s, "measurements.csv"), newline="") as f:
                for row in csv.DictReader(f):
                    paths.append(os.path.join(data_dir, s, "images", row["image_filename"]))
                    for k in cols:
                        cols[k].append(float(row[k]))
                    if row["command_name"] not in COMMAND_MAP:
                        raise RuntimeError(f"unknown command_name {row['command_name']!r} in {s}")
                    cmds.append(COMMAND_MAP[row["command_name"]])
        self.paths = np.array(paths, dtype=object)
        self.targets = np.stack([np.array(cols[k], dtype=np.float32)
                                 for k in ("steer", "throttle", "brake")], axis=1)
        self.speed = np.array(cols["speed_normalized"], dtype=np.float32)
        self.command = np.array(cmds, dtype=np.int64)

    def __len__(self):
        return len(self.paths)

    def split(self, test_size=0.15, random_state=42):
        """The reference's stratified split (notebook.ipynb:376-377) -> (train_idx, val_idx)."""
        from sklearn.model_selection import train_test_split
        idx = np.arange(len(self))
        tr, va = train_test_split(idx, test_size=test_size, random_state=random_state,
                                  stratify=self.command)
        return tr, va


def drive_ranges(sessions: "Sessions", max_gap: int = 1) -> list:
    """[(begin, end), ...]: the half-open index ranges of `sessions` that are one unbroken drive.
    A range ends where the session directory changes and wherever the frame number in
    `frame_%08d.jpg` moves by anything but 1 .. max_gap: the recorder does not save the frames it
    skips as stuck (model/collect_data.py), so a session is not one drive.  What
    `evaluate.replay` replays must lie inside one range; the starts are the caller's choice."""
    import re
    if max_gap < 1:
        raise ValueError("drive_ranges: max_gap must be at least 1")
    keys = []
    for p in sessions.paths:
        m = re.fullmatch(r"frame_(\d+)\.\w+", os.path.basename(p))
        if m is None:
            raise RuntimeError(f"drive_ranges: no frame number in {p!r}")
        keys.append((os.path.dirname(os.path.dirname(p)), int(m.group(1))))
    out, begin = [], 0
    for i in range(1, len(keys) + 1):
        if i == len(keys) or keys[i][0] != keys[i - 1][0] \
                or not (1 <= keys[i][1] - keys[i - 1][1] <= max_gap):
            out.append((begin, i))
            begin = i
    return out


def class_balanced_weights(command: np.ndarray) -> np.ndarray:
    """Per-sample weight len / (4 * count[command]) (notebook.ipynb:383-384, 421)."""
    counts = np.bincount(command, minlength=4).astype(np.float64)
    cw = len(command) / (4.0 * np.where(counts > 0, counts, 1.0))
    return cw[command]


def weighted_indices(weights: np.ndarray, num_samples: int, generator=None) -> torch.Tensor:
    """WeightedRandomSampler(weights, num_samples, replacement=True) (notebook.ipynb:422-423):
    torch.multinomial over the double weights."""
    return torch.multinomial(torch.as_tensor(weights, dtype=torch.double), num_samples, True,
                             generator=generator)


def decode_jpeg(path: str) -> np.ndarray:
    """cv2.imread + BGR2RGB (notebook.ipynb:408-409) -> uint8 RGB [H,W,3]."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class BatchLoader:
    """Iterates (image, speed, command, targets) device batches like the reference's DataLoader
    (notebook.ipynb:428-431).  train=True: class-balanced sampling with replacement, device-side
    augmentation, drop_last; train=False: sequential, no augmentation, last partial batch kept.
    JPEGs are decoded by `workers` threads into pinned memory one batch ahead of the consumer."""

    def __init__(self, sessions: Sessions, indices, batch_size: int, device, train: bool,
                 seed: int = 0, workers: int = 8, height: int = IMG_HEIGHT, width: int = IMG_WIDTH,
                 processes: bool = False, rank: int = 0, world_size: int = 1,
                 weather: "WeatherMix" = None, view: "ViewShift" = None):
        """processes=True decodes in `workers` spawned processes (no GIL contention: what a
        B=128 / 14 ms training step needs); the default thread pool starts instantly.

        Data parallel (rank, world_size): every rank draws the SAME epoch order from the shared
        sampler stream (same `seed`) and keeps every world_size-th index starting at `rank`
        (SURVEY.md 8e "rank-strided sampling"): the ranks' index sets are disjoint and their
        union is exactly the single-process draw, so N ranks x batch B consume what one process
        at batch N*B would.  The order is cut to a multiple of world_size * batch_size when
        training (drop_last on the GLOBAL batch) so every rank runs the same number of steps --
        a rank with one batch more would hang the others' all-reduce.  Augmentation parameters
        come from a rank-offset stream.

        weather: a `WeatherMix`; every sample's weather record is drawn batch by batch from a
        stream of its own and applied in the augmentation launch (train or not).  The sample order
        and the augmentation records are those of the same loader without it; None launches the
        plain kernel.

        view: a `ViewShift`; every sample's viewpoint record is drawn batch by batch from a third
        stream of its own (its speed feeds the steering rule), the steer labels are corrected on
        the host with the kernel's float32 add and clip, and the frames are warped in the same
        launch, in front of the weather.  Order, augmentation and weather records are unchanged."""
        if not (0 <= rank < world_size):
            raise ValueError(f"rank {rank} outside world of {world_size}")
        self.s, self.idx = sessions, np.asarray(indices)
        self.bs, self.device, self.train = batch_size, torch.device(device), train
        self.h, self.w = height, width
        self.rank, self.world = rank, world_size
        self.rng = np.random.default_rng([seed, rank])
        self.weather = weather
        self.wrng = np.random.default_rng([seed, rank, WEATHER_STREAM])
        self.view = view
        self.vrng = np.random.default_rng([seed, rank, VIEW_STREAM])
        self.gen = torch.Generator().manual_seed(seed)
        self.workers = max(1, workers)
        self.processes = processes
        self.pool = None
        self._slots = None
        self.weights = class_balanced_weights(sessions.command[self.idx]) if train else None

    def _ensure_pool(self):
        if self.pool is None:
            if self.processes:
                import multiprocessing as mp
                self.pool = mp.get_context("spawn").Pool(self.workers)
            else:
                from multiprocessing.pool import ThreadPool
                self.pool = ThreadPool(self.workers)
        return self.pool

    def close(self):
        if self.pool is not None:
            self.pool.terminate()
            self.pool.join()
            self.pool = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shard_len(self):
        n = len(self.idx)
        if self.train:
            return n // (self.bs * self.world) * self.bs
        return len(range(self.rank, n, self.world))

    def __len__(self):
        n = self._shard_len()
        return n // self.bs if self.train else (n + self.bs - 1) // self.bs

    def _order(self):
        """This rank's sample order for one epoch (see __init__ for the sharding rule)."""
        if self.train:
            pick = weighted_indices(self.weights, len(self.idx), self.gen).numpy()
            order = self.idx[pick]
            order = order[:len(order) // (self.bs * self.world) * self.bs * self.world]
        else:
            order = self.idx
        return order[self.rank::self.world]

    def __iter__(self):
        try:
            from cilrs_jpeg_worker import decode_chunk
        except ImportError:          # the worker module sits next to the package directory
            import sys
            sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            from cilrs_jpeg_worker import decode_chunk
        order = self._order()
        nb = len(self)
        q: queue.Queue = queue.Queue(maxsize=3)
        pool = self._ensure_pool()
        chunk = max(4, -(-self.bs // self.workers))
        batches = [order[b * self.bs:(b + 1) * self.bs] for b in range(nb)]

        def tasks():              # every batch cut into per-worker chunks, in order
            for ids in batches:
                for c in range(0, len(ids), chunk):
                    yield (list(self.s.paths[ids[c:c + chunk]]), self.h, self.w)

        # ring of pinned staging buffers, allocated (and touched) once: a fresh pinned allocation
        # costs ~15 ms and its first DMA another ~17 ms on this platform (tools/loader_probe.py)
        if self._slots is None:
            self._slots = []
            for _ in range(4):
                t = torch.zeros(self.bs, self.h, self.w, 3, dtype=torch.uint8).pin_memory()
                meta = (torch.zeros(self.bs, dtype=torch.float32).pin_memory(),
                        torch.zeros(self.bs, dtype=torch.int64).pin_memory(),
                        torch.zeros(self.bs, 3, dtype=torch.float32).pin_memory(),
                        torch.zeros(self.bs, AUG_DTYPE.itemsize, dtype=torch.uint8).pin_memory(),
                        torch.zeros(self.bs, WEATHER_DTYPE.itemsize, dtype=torch.uint8).pin_memory(),
                        torch.zeros(self.bs, VIEW_DTYPE.itemsize, dtype=torch.uint8).pin_memory())
                self._slots.append((t, t.numpy(), meta))
            # host-to-device copies run on a stream of their own: the wait that frees a staging
            # slot then waits for the COPY, not for the train step the copy would otherwise queue
            # behind (with everything on one stream the host could never run ahead of the device:
            # 12.6 k frames/s feeding a 13.9 k frames/s step)
            self._copy_stream = torch.cuda.Stream(device=self.device) \
                if torch.device(self.device).type == "cuda" else None
        free: queue.Queue = queue.Queue()
        for k in range(len(self._slots)):
            free.put(k)

        def producer():
            try:
                results = pool.imap(decode_chunk, tasks())       # ordered, workers run ahead
                for ids in batches:
                    slot = free.get()
                    view = self._slots[slot][1]
                    k = 0
                    while k < len(ids):
                        part = next(results)
                        view[k:k + len(part)] = part
                        k += len(part)
                    params = draw_aug_params(self.rng, len(ids), self.h, self.w) if self.train \
                        else identity_params(len(ids))
                    wrec = self.weather.draw(self.wrng, len(ids), self.h, self.w) \
                        if self.weather is not None else None
                    vrec = self.view.draw(self.vrng, len(ids), self.s.speed[ids], self.h, self.w) \
                        if self.view is not None else None
                    q.put((slot, params, wrec, vrec, ids))
                q.put(None)
            except Exception as e:          # surface decode errors in the consumer
                q.put(e)
        threading.Thread(target=producer, daemon=True).start()
        while True:
            item = q.get()
            if item is None:
                return
            if isinstance(item, Exception):
                raise item
            slot, params, wrec, vrec, ids = item
            n = len(ids)
            pinned, _view, (sp_p, cm_p, tg_p, par_p, wx_p, vw_p) = self._slots[slot]
            par_p[:n] = torch.from_numpy(params.view(np.uint8).reshape(n, AUG_DTYPE.itemsize))
            if wrec is not None:
                wx_p[:n] = torch.from_numpy(wrec.view(np.uint8).reshape(n, WEATHER_DTYPE.itemsize))
            sp_p[:n] = torch.from_numpy(np.ascontiguousarray(self.s.speed[ids], dtype=np.float32))
            cm_p[:n] = torch.from_numpy(np.ascontiguousarray(self.s.command[ids], dtype=np.int64))
            tgt = np.ascontiguousarray(self.s.targets[ids], dtype=np.float32)
            if vrec is not None:
                vw_p[:n] = torch.from_numpy(vrec.view(np.uint8).reshape(n, VIEW_DTYPE.itemsize))
                tgt = correct_steer(tgt, vrec)
            tg_p[:n] = torch.from_numpy(tgt)
            cs = self._copy_stream
            main = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(cs):
                frames = torch.empty(n, self.h, self.w, 3, dtype=torch.uint8, device=self.device)
                frames.copy_(pinned[:n], non_blocking=True)
                speeds = sp_p[:n].to(self.device, non_blocking=True)
                cmds = cm_p[:n].to(self.device, non_blocking=True)
                tgts = tg_p[:n].to(self.device, non_blocking=True)
                pars = par_p[:n].to(self.device, non_blocking=True)
                wxs = wx_p[:n].to(self.device, non_blocking=True) if wrec is not None else None
                vws = vw_p[:n].to(self.device, non_blocking=True) if vrec is not None else None
                copied = torch.cuda.Event()
                copied.record(cs)
            main.wait_event(copied)          # device side: the consumers run behind the copies
            for t in (frames, speeds, cmds, tgts, pars, wxs, vws):
                if t is not None:
                    t.record_stream(main)    # (allocated under the copy stream, used on `main`)
            img = augment_u8(frames, params, params_dev=pars, weather=wrec, weather_dev=wxs,
                             view=vrec, view_dev=vws)
            batch = (img, speeds, cmds, tgts)
            copied.synchronize()            # the staging slot may be refilled now
            free.put(slot)
            yield batch


# ---- device-resident dataset -----------------------------------------------------------------
def _decode_chunk():
    try:
        from cilrs_jpeg_worker import decode_chunk
    except ImportError:          # the worker module sits next to the package directory
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from cilrs_jpeg_worker import decode_chunk
    return decode_chunk


class DeviceDataset:
    """Every decoded frame of a `Sessions` plus its labels on one device: the JPEGs are decoded
    ONCE (`fill`) and each batch is then built there by one `cilrs_batch_assemble` launch
    (`assemble`, `CachedBatchLoader`) -- no decode, staging buffer or host-to-device copy per step.

    The whole dataset must fit: `cache_bytes(n, h, w)` against `budget_bytes` (default: half of
    the device memory free at construction) is checked before anything is allocated or decoded.
    There is no partial cache; a dataset over budget is `BatchLoader`'s job."""

    LABEL_BYTES = 4 + 8 + 12          # speed f32, command i64, targets f32 [3] per frame

    @staticmethod
    def cache_bytes(n: int, h: int = IMG_HEIGHT, w: int = IMG_WIDTH) -> int:
        """Device bytes the cache of n frames takes: the uint8 frames and the label arrays."""
        return int(n) * (int(h) * int(w) * 3 + DeviceDataset.LABEL_BYTES)

    def __init__(self, sessions: Sessions, device, height: int = IMG_HEIGHT,
                 width: int = IMG_WIDTH, budget_bytes: int = None, workers: int = 8,
                 processes: bool = False, chunk_frames: int = 1024, fill: bool = True,
                 process_group=None, mem_get_info=None):
        """workers / processes: the decode pool, as in `BatchLoader`.  chunk_frames: frames per
        pinned staging buffer (and, filling data-parallel, per collective).  fill=False leaves
        the cache unallocated until `fill()` is called.  mem_get_info: stands in for
        `torch.cuda.mem_get_info` (device -> (free, total) bytes)."""
        self.s = sessions
        self.n, self.h, self.w = len(sessions), height, width
        self.device = torch.device(device)
        self.workers, self.processes = max(1, workers), processes
        self.chunk_frames = max(1, chunk_frames)
        self.command = sessions.command           # host copy: the sampler's class weights
        self.speed_host = getattr(sessions, "speed", None)    # host copy: the steering rule's
        self.cache = self.speed = self.command_dev = self.targets = None
        need = self.cache_bytes(self.n, height, width)
        if budget_bytes is None:
            free = (mem_get_info or torch.cuda.mem_get_info)(self.device)[0]
            budget_bytes = free // 2
        self.budget_bytes = int(budget_bytes)
        if need > self.budget_bytes:
            raise RuntimeError(
                f"DeviceDataset: {self.n} frames of {width}x{height} need {need} bytes on the "
                f"device, the budget is {self.budget_bytes} bytes; use BatchLoader (decode per "
                "epoch) for a dataset that does not fit")
        if fill:
            self.fill(process_group)

    @classmethod
    def from_tensors(cls, cache: torch.Tensor, speed: torch.Tensor, command: torch.Tensor,
                     targets: torch.Tensor):
        """A dataset over frames and labels that are on the device already (uint8 [N,H,W,3],
        f32 [N], i64 [N], f32 [N,3]); the tensors are used as they are, not copied."""
        n = cache.size(0) if cache.dim() == 4 else -1
        ok = cache.dtype == torch.uint8 and cache.dim() == 4 and cache.size(3) == 3 and n >= 1 \
            and cache.device.type == "cuda" and cache.is_contiguous()
        for t, dt, shape in ((speed, torch.float32, (n,)), (command, torch.int64, (n,)),
                             (targets, torch.float32, (n, 3))):
            ok = ok and t.dtype == dt and tuple(t.shape) == shape and t.device == cache.device \
                and t.is_contiguous()
        if not ok:
            raise RuntimeError("DeviceDataset.from_tensors: need contiguous uint8 [N,H,W,3] frames, "
                               "f32 [N] speed, i64 [N] command and f32 [N,3] targets on one GPU")
        self = cls.__new__(cls)
        self.s = None
        self.n, self.h, self.w = n, cache.size(1), cache.size(2)
        self.device = cache.device
        self.command = command.cpu().numpy()
        self.speed_host = speed.cpu().numpy()
        self.cache, self.speed, self.command_dev, self.targets = cache, speed, command, targets
        self.budget_bytes = None
        return self

    def __len__(self):
        return self.n

    @property
    def filled(self):
        return self.cache is not None

    def fill(self, process_group=None):
        """Decode every frame once and copy it to the device through pinned staging buffers.

        process_group (world W > 1): rank r decodes frames r, r+W, r+2W, ... only and the ranks
        all-gather their shares chunk by chunk, so every rank ends with the full cache, byte for
        byte what a single-process fill gives (the sampler draws from the whole dataset on every
        rank).  A gloo group exchanges the pinned host buffers themselves; any other backend the
        uploaded shares."""
        if self.device.type != "cuda":
            raise RuntimeError("DeviceDataset: the cache lives on a GPU (no CPU fallback)")
        rank, world, on_host = 0, 1, True
        if process_group is not None:
            import torch.distributed as dist
            rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
            on_host = "gloo" in str(dist.get_backend(process_group))
        decode_chunk = _decode_chunk()
        n, h, w, dev, s = self.n, self.h, self.w, self.device, self.s
        share = -(-n // world)                      # frames rank 0 decodes; no rank has more
        K = min(self.chunk_frames, share)           # frames per staging buffer
        rounds = -(-share // K)                     # the same on every rank
        cache = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
        speed = torch.from_numpy(np.ascontiguousarray(s.speed, dtype=np.float32)).to(dev)
        command = torch.from_numpy(np.ascontiguousarray(s.command, dtype=np.int64)).to(dev)
        targets = torch.from_numpy(np.ascontiguousarray(s.targets, dtype=np.float32)).to(dev)
        mine = np.arange(rank, n, world)
        piece = max(4, min(64, -(-K // self.workers)))

        def tasks():
            for c in range(rounds):
                ids = mine[c * K:(c + 1) * K]
                for k in range(0, len(ids), piece):
                    yield (list(s.paths[ids[k:k + piece]]), h, w)

        if self.processes:
            import multiprocessing as mp
            pool = mp.get_context("spawn").Pool(self.workers)
        else:
            from multiprocessing.pool import ThreadPool
            pool = ThreadPool(self.workers)
        stream = torch.cuda.current_stream(dev)
        # two staging slots: the pool decodes into one while the other's copies are in flight
        nslot = 2 if rounds > 1 else 1
        slots = []
        for _ in range(nslot):
            send = torch.zeros(K, h, w, 3, dtype=torch.uint8).pin_memory()
            recv = None
            if world > 1:
                recv = [torch.zeros(K, h, w, 3, dtype=torch.uint8).pin_memory() if on_host
                        else torch.empty(K, h, w, 3, dtype=torch.uint8, device=dev)
                        for _ in range(world)]
            slots.append([send, send.numpy(), recv, None])
        try:
            results = pool.imap(decode_chunk, tasks())       # ordered, workers run ahead
            for c in range(rounds):
                slot = slots[c % nslot]
                send, view, recv, done = slot
                if done is not None:
                    done.synchronize()                       # the slot's last copies have left it
                ids = mine[c * K:(c + 1) * K]
                k = 0
                while k < len(ids):
                    part = next(results)                     # a decode error surfaces here
                    view[k:k + len(part)] = part
                    k += len(part)
                if world == 1:
                    cache[c * K:c * K + len(ids)].copy_(send[:len(ids)], non_blocking=True)
                else:
                    import torch.distributed as dist
                    if on_host:
                        dist.all_gather(recv, send, group=process_group)
                    else:
                        dist.all_gather(recv, send.to(dev, non_blocking=True), group=process_group)
                    for q in range(world):                   # rank q's share: q + W * (cK ...)
                        first = q + world * c * K
                        cnt = len(range(first, min(n, first + world * K), world))
                        if cnt > 0:
                            cache[first:first + world * cnt:world].copy_(recv[q][:cnt],
                                                                         non_blocking=True)
                done = torch.cuda.Event()
                done.record(stream)
                slot[3] = done
            stream.synchronize()
        finally:
            pool.terminate()
            pool.join()
        self.cache, self.speed, self.command_dev, self.targets = cache, speed, command, targets
        return self

    def check_index(self, index: np.ndarray):
        """Host check of the kernel's contract: every value in [0, n)."""
        if index.size and (int(index.min()) < 0 or int(index.max()) >= self.n):
            bad = index[(index < 0) | (index >= self.n)][0]
            raise RuntimeError(f"DeviceDataset: index {int(bad)} outside [0, {self.n})")

    def _launch(self, index_ptr: int, params_ptr: int, b: int, want_u8: bool = False,
                weather_ptr: int = None, view_ptr: int = None):
        """One cilrs_batch_assemble launch on the current stream from device-resident index /
        parameter records (already checked on the host); with weather_ptr (device-resident
        weather records), one cilrs_batch_assemble_weather launch; with view_ptr (device-resident
        viewpoint records), one cilrs_batch_assemble_view launch, with or without weather."""
        dev = self.device
        out = torch.empty(b, self.h, self.w, 3, dtype=torch.float32, device=dev)
        out8 = torch.empty(b, self.h, self.w, 3, dtype=torch.uint8, device=dev) if want_u8 else None
        spd = torch.empty(b, dtype=torch.float32, device=dev)
        cmd = torch.empty(b, dtype=torch.int64, device=dev)
        tgt = torch.empty(b, 3, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        if view_ptr is not None:
            L.check(L.lib().cilrs_batch_assemble_view(
                L.ptr(self.cache), self.n, L.ptr(self.speed), L.ptr(self.command_dev),
                L.ptr(self.targets), C.c_void_p(index_ptr), C.c_void_p(params_ptr),
                C.c_void_p(weather_ptr), C.c_void_p(view_ptr), b, self.h, self.w, L.ptr(out),
                L.ptr(out8), L.ptr(spd), L.ptr(cmd), L.ptr(tgt), C.c_void_p(stream)))
        elif weather_ptr is None:
            L.check(L.lib().cilrs_batch_assemble(
                L.ptr(self.cache), self.n, L.ptr(self.speed), L.ptr(self.command_dev),
                L.ptr(self.targets), C.c_void_p(index_ptr), C.c_void_p(params_ptr), b, self.h,
                self.w, L.ptr(out), L.ptr(out8), L.ptr(spd), L.ptr(cmd), L.ptr(tgt),
                C.c_void_p(stream)))
        else:
            L.check(L.lib().cilrs_batch_assemble_weather(
                L.ptr(self.cache), self.n, L.ptr(self.speed), L.ptr(self.command_dev),
                L.ptr(self.targets), C.c_void_p(index_ptr), C.c_void_p(params_ptr),
                C.c_void_p(weather_ptr), b, self.h, self.w, L.ptr(out), L.ptr(out8), L.ptr(spd),
                L.ptr(cmd), L.ptr(tgt), C.c_void_p(stream)))
        img = out.permute(0, 3, 1, 2)              # the NCHW view `augment_u8` returns
        return (img, spd, cmd, tgt, out8) if want_u8 else (img, spd, cmd, tgt)

    def assemble(self, index, params: np.ndarray, want_u8: bool = False,
                 weather: np.ndarray = None, view: np.ndarray = None):
        """index (host integers [B], any order, repeats allowed) + one parameter record per sample
        -> (image, speed, command, targets[, augmented uint8 frames]) on the device: what
        `augment_u8(cache[index], params)` and an index_select of the labels give.  The index is
        checked on the host before anything is launched.  weather: one WEATHER_DTYPE record per
        sample, applied to the source frames in the same launch (`augment_u8(..., weather=)`).
        view: one VIEW_DTYPE record per sample; the frames are seen from those viewpoints first and
        the steer targets corrected, in the same launch (`cilrs_batch_assemble_view`)."""
        if isinstance(index, torch.Tensor):
            index = index.cpu().numpy()
        index = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
        self.check_index(index)
        if index.size < 1:
            raise RuntimeError("DeviceDataset.assemble: empty index")
        if params.shape != index.shape:
            raise RuntimeError("DeviceDataset.assemble: one parameter record per index")
        check_params(params, self.h, self.w)
        if weather is not None:
            if not isinstance(weather, np.ndarray) or weather.shape != index.shape:
                raise RuntimeError("DeviceDataset.assemble: one weather record per index")
            check_weather(weather, self.h, self.w)
        if view is not None:
            if not isinstance(view, np.ndarray) or view.shape != index.shape:
                raise RuntimeError("DeviceDataset.assemble: one view record per index")
            check_view(view, self.h, self.w)
        if not self.filled:
            raise RuntimeError("DeviceDataset.assemble: the cache is not filled (call fill())")
        b = index.size
        idx_dev = torch.from_numpy(index).to(self.device)
        par_dev = torch.from_numpy(params.view(np.uint8).reshape(b, AUG_DTYPE.itemsize)).to(
            self.device)
        wx_dev = _records_to_device(weather, self.device) if weather is not None else None
        vw_dev = _records_to_device(view, self.device) if view is not None else None
        res = self._launch(idx_dev.data_ptr(), par_dev.data_ptr(), b, want_u8,
                           wx_dev.data_ptr() if wx_dev is not None else None,
                           vw_dev.data_ptr() if vw_dev is not None else None)
        for t in (idx_dev, par_dev, wx_dev, vw_dev):
            if t is not None:
                t.record_stream(torch.cuda.current_stream(self.device))
        return res


class _Ahead:
    """fn() on a background thread; result() joins it and re-raises what it raised."""

    def __init__(self, fn):
        self.out = self.err = None
        self.thread = threading.Thread(target=self._run, args=(fn,), daemon=True)
        self.thread.start()

    def _run(self, fn):
        try:
            self.out = fn()
        except Exception as e:           # re-raised by result(), in the consumer
            self.err = e

    def result(self):
        self.thread.join()
        if self.err is not None:
            raise self.err
        return self.out


class CachedBatchLoader:
    """`BatchLoader` over a `DeviceDataset`: the same arguments, the same batches bit for bit for
    the same (seed, rank, world_size, batch_size, train) -- the epoch order comes from the same
    `torch.Generator` stream, the augmentation parameters from the same
    `np.random.default_rng([seed, rank])` stream drawn batch by batch, and both carry over from
    epoch to epoch.  The whole epoch's order and parameters (120 bytes a sample) go to the device
    once when the epoch starts; each batch is then one kernel launch on the current stream, with
    no copy, pinned ring, event wait or host synchronisation per step.  Drawing a training
    epoch's parameters is host work of a few hundred microseconds a batch, so while one epoch
    runs the next one's plan is drawn on a background thread: the device does not idle at the
    epoch boundary.

    weather (a `WeatherMix`): as for `BatchLoader`, from the same stream of its own, so the two
    loaders stay bit-identical with it; the epoch's weather records (96 bytes a sample) are drawn
    with the plan and go up with it, and every batch is one `cilrs_batch_assemble_weather`
    launch.  train=False with a mix scores a validation set under that weather.

    view (a `ViewShift`): likewise from a third stream; the dataset's host copy of the speeds
    (`speed_host`) feeds the steering rule, the epoch's viewpoint records (96 bytes a sample) go up
    with the plan, and every batch is one `cilrs_batch_assemble_view` launch that warps the frames
    and corrects the steer labels.  train=False with a mix scores a validation set from the
    shifted viewpoint."""

    def __init__(self, dataset, indices, batch_size: int, train: bool, seed: int = 0,
                 rank: int = 0, world_size: int = 1, weather: "WeatherMix" = None,
                 view: "ViewShift" = None):
        if not (0 <= rank < world_size):
            raise ValueError(f"rank {rank} outside world of {world_size}")
        self.ds, self.idx = dataset, np.asarray(indices)
        self.bs, self.train = batch_size, train
        self.h = getattr(dataset, "h", IMG_HEIGHT)
        self.w = getattr(dataset, "w", IMG_WIDTH)
        self.rank, self.world = rank, world_size
        self.rng = np.random.default_rng([seed, rank])
        self.weather = weather
        self.wrng = np.random.default_rng([seed, rank, WEATHER_STREAM])
        self.view = view
        self.vrng = np.random.default_rng([seed, rank, VIEW_STREAM])
        if view is not None and getattr(dataset, "speed_host", None) is None:
            raise RuntimeError("CachedBatchLoader: view= needs the dataset's host speeds "
                               "(speed_host)")
        self.gen = torch.Generator().manual_seed(seed)
        self.weights = class_balanced_weights(dataset.command[self.idx]) if train else None
        self._ahead = None

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    _shard_len = BatchLoader._shard_len
    __len__ = BatchLoader.__len__
    _order = BatchLoader._order

    def epoch_plan(self):
        """(order, params) of the next epoch, on the host: this rank's sample order (int64 [n])
        and the augmentation records of its batches back to back (AUG_DTYPE [n]); with a weather
        mix (order, params, weather), the weather records (WEATHER_DTYPE [n]) follow, and with a
        view mix the viewpoint records (VIEW_DTYPE [n]) come last.  Touches no GPU; advances the
        sampler, parameter, weather and viewpoint streams exactly as one `BatchLoader` epoch does.
        Successive calls, by the caller or by iteration, give successive epochs: a plan already
        drawn ahead (`_plan_ahead`) is handed out before a new one is drawn."""
        order, params, weather, view = self._next_plan()
        return (order, params) + (() if self.weather is None else (weather,)) \
            + (() if self.view is None else (view,))

    def _next_plan(self):
        ahead, self._ahead = self._ahead, None
        return ahead.result() if ahead is not None else self._draw_plan()

    def _plan_ahead(self):
        """Start drawing the next epoch's plan on a background thread."""
        if self._ahead is None:
            self._ahead = _Ahead(self._draw_plan)

    def _draw_plan(self):
        order = np.ascontiguousarray(self._order(), dtype=np.int64)
        nb = len(self)
        order = order[:nb * self.bs]
        parts, wparts, vparts = [], [], []
        for b in range(nb):
            n = len(order[b * self.bs:(b + 1) * self.bs])
            parts.append(draw_aug_params(self.rng, n, self.h, self.w) if self.train
                         else identity_params(n))
            if self.weather is not None:
                wparts.append(self.weather.draw(self.wrng, n, self.h, self.w))
            if self.view is not None:
                ids = order[b * self.bs:(b + 1) * self.bs]
                vparts.append(self.view.draw(self.vrng, n, self.ds.speed_host[ids], self.h, self.w))
        params = np.concatenate(parts) if parts else np.zeros(0, dtype=AUG_DTYPE)
        weather = None
        if self.weather is not None:
            weather = np.concatenate(wparts) if wparts else np.zeros(0, dtype=WEATHER_DTYPE)
        view = None
        if self.view is not None:
            view = np.concatenate(vparts) if vparts else np.zeros(0, dtype=VIEW_DTYPE)
        return order, params, weather, view

    def __iter__(self):
        ds = self.ds
        order, params, weather, view = self._next_plan()
        ds.check_index(order)
        check_params(params, self.h, self.w)
        if weather is not None:
            check_weather(weather, self.h, self.w)
        if view is not None:
            check_view(view, self.h, self.w)
        if not ds.filled:
            raise RuntimeError("CachedBatchLoader: the dataset's cache is not filled")
        n = len(order)
        if n == 0:
            return
        # pinned, so the two uploads are asynchronous; the caching host allocator keeps the pinned
        # blocks until the copies have run
        order_dev = torch.from_numpy(order).pin_memory().to(ds.device, non_blocking=True)
        params_dev = torch.from_numpy(params.view(np.uint8).reshape(n, AUG_DTYPE.itemsize)) \
            .pin_memory().to(ds.device, non_blocking=True)
        weather_dev = None
        if weather is not None:
            weather_dev = torch.from_numpy(weather.view(np.uint8).reshape(
                n, WEATHER_DTYPE.itemsize)).pin_memory().to(ds.device, non_blocking=True)
        view_dev = None
        if view is not None:
            view_dev = torch.from_numpy(view.view(np.uint8).reshape(
                n, VIEW_DTYPE.itemsize)).pin_memory().to(ds.device, non_blocking=True)
        if self.train:
            self._plan_ahead()
        ip, pp = order_dev.data_ptr(), params_dev.data_ptr()
        wp = weather_dev.data_ptr() if weather_dev is not None else None
        vp = view_dev.data_ptr() if view_dev is not None else None
        for b0 in range(0, n, self.bs):
            yield ds._launch(ip + b0 * 8, pp + b0 * AUG_DTYPE.itemsize, min(self.bs, n - b0),
                             weather_ptr=None if wp is None else wp + b0 * WEATHER_DTYPE.itemsize,
                             view_ptr=None if vp is None else vp + b0 * VIEW_DTYPE.itemsize)
