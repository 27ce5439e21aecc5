"""float32 numpy restatement of the weather stages (TEST INFRASTRUCTURE ONLY): tone, fog and rain
as include/cilrs_hip.h defines them, one rounding per operation in the order csrc/augment.hip
performs them, on uint8 frames.  It composes with `augment_oracle.augment_batch` for the stages
behind it: weather is a function of the source pixel, so the kernels must give what the plain
augmentation gives on `weather_batch(frames, records)`.

A record is one element of a `data.WEATHER_DTYPE` array (or a dict with the same field names)."""
import numpy as np

import augment_oracle as AO

F = np.float32


def _clip255(x):
    return np.minimum(np.maximum(x, F(0)), F(255))


def fog_depth(height, horizon, near):
    """flat-ground pseudo-depth of every row, float32 [H], in (0, 1]"""
    yf = np.arange(height).astype(F)
    hz, nr = F(horizon), F(near)
    below = nr / np.maximum(yf - hz, nr)
    return np.where(yf <= hz, F(1), below).astype(F)


def fog_transmission(w, height):
    """t = clip(t0 + t1 * d, 0, 1) per row, float32 [H]"""
    d = fog_depth(height, w["fog_horizon"], w["fog_near"])
    t = F(w["fog_t1"]) * d
    t = F(w["fog_t0"]) + t
    return np.minimum(np.maximum(t, F(0)), F(1)).astype(F)


def rain_heads(seed, yy, xx, thresh24):
    """streak-head predicate at integer positions (arrays of equal shape, may lie off the frame)"""
    with np.errstate(over="ignore"):
        e = (yy + 64).astype(np.uint64) * np.uint64(65536) + (xx + 64).astype(np.uint64)
        h = AO._splitmix64(np.uint64(seed) + e * np.uint64(0xD1B54A32D192ED03))
    return (h >> np.uint64(40)) < np.uint64(thresh24)


def rain_cover(w, height, width):
    """smallest covering tail position per pixel, int [H, W]; rain_len where uncovered"""
    L, slant = int(w["rain_len"]), int(w["rain_slant_q4"])
    y = np.arange(height)[:, None]
    x = np.arange(width)[None, :]
    jmin = np.full((height, width), L, dtype=np.int64)
    for j in range(L - 1, -1, -1):
        off = (j * slant) >> 4                      # arithmetic shift: a floor
        hd = rain_heads(w["rain_seed"], np.broadcast_to(y - j, (height, width)),
                        np.broadcast_to(x - off, (height, width)), int(w["rain_thresh24"]))
        jmin = np.where(hd, j, jmin)
    return jmin


def weather_one(frame_u8, w):
    """uint8 [H,W,3] + one record -> uint8 [H,W,3]"""
    H, W = frame_u8.shape[:2]
    c = frame_u8.astype(F)
    if int(w["tone_on"]):
        t = c * np.asarray(w["gain"], dtype=F)
        t = t + np.asarray(w["lift255"], dtype=F)
        c = np.trunc(_clip255(t))
    if int(w["fog_on"]):
        t = fog_transmission(w, H)[:, None, None]
        A = np.asarray(w["fog_rgb255"], dtype=F)
        u = c - A
        u = u * t
        u = A + u
        c = np.rint(_clip255(u))
    L = int(w["rain_len"])
    if L > 0:
        jmin = rain_cover(w, H, W)
        a = (F(L) - jmin.astype(F)) / F(L)
        a = (F(w["rain_alpha"]) * a)[..., None]
        u = F(w["rain_v255"]) - c
        u = a * u
        u = c + u
        c = np.where((jmin < L)[..., None], np.rint(_clip255(u)), c)
    return c.astype(np.uint8)


def weather_batch(frames_u8, records):
    return np.stack([weather_one(f, w) for f, w in zip(frames_u8, records)])


def aug_recs(p):
    """AUG_DTYPE array -> the list of dicts augment_oracle takes"""
    return [{k: (r[k].tolist() if hasattr(r[k], "tolist") else r[k]) for k in p.dtype.names}
            for r in p]


def augment_weather_batch(frames_u8, params, records):
    """what cilrs_augment_weather_u8 must give: (uint8 [B,H,W,3], normalised float32 [B,H,W,3])"""
    return AO.augment_batch(weather_batch(frames_u8, records), aug_recs(params))
