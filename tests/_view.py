"""float32 numpy restatement of the viewpoint warp (TEST INFRASTRUCTURE ONLY): the virtual frame V
as include/cilrs_hip.h defines it, one rounding per operation in the order csrc/augment.hip
performs them, on uint8 frames.  It composes with `_weather.weather_batch` and
`augment_oracle.augment_batch` for the stages behind it: the warp is a function of the stored
frame alone, so the kernels must give what the weather / plain augmentation gives on
`view_batch(frames, records)`.

Also a float64 pinhole projector written from dot products with the camera's axes, independently
of `data.view_records`, for the geometry tests.

A record is one element of a `data.VIEW_DTYPE` array (or a dict with the same field names)."""
import numpy as np

import _weather as WX
import augment_oracle as AO

F = np.float32


def _clip255(x):
    return np.minimum(np.maximum(x, F(0)), F(255))


def source_coords(v, H, W):
    """(sx, sy) float32 [H, W]: the clamped source position of every destination pixel"""
    y = np.arange(H).astype(F)[:, None]
    x = np.arange(W).astype(F)[None, :]
    ground = y > F(v["split_row"])
    far, gr = np.asarray(v["far"], dtype=F), np.asarray(v["ground"], dtype=F)
    M = [np.where(ground, gr[i], far[i]).astype(F) for i in range(9)]      # [H, 1] each
    with np.errstate(all="ignore"):
        u = (M[0] * x + M[1] * y) + M[2]
        t = (M[3] * x + M[4] * y) + M[5]
        w = (M[6] * x + M[7] * y) + M[8]
        # fmax / fmin return the other operand for a NaN, as fmaxf / fminf do: a NaN goes to 0
        sx = np.fmin(np.fmax(u / w, F(0)), F(W - 1))
        sy = np.fmin(np.fmax(t / w, F(0)), F(H - 1))
    assert sx.dtype == F and sy.dtype == F
    return sx, sy


def view_one(frame_u8, v):
    """uint8 [H,W,3] + one record -> uint8 [H,W,3]"""
    if not int(v["on"]):
        return frame_u8.copy()
    H, W = frame_u8.shape[:2]
    sx, sy = source_coords(v, H, W)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    ax, ay = (sx - x0.astype(F))[..., None], (sy - y0.astype(F))[..., None]
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    # numpy would wrap a negative index silently: no address outside the frame, stated
    assert x0.min() >= 0 and x1.max() <= W - 1 and y0.min() >= 0 and y1.max() <= H - 1
    p = frame_u8.astype(F)
    p00, p01, p10, p11 = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
    top = p00 + ax * (p01 - p00)
    bot = p10 + ax * (p11 - p10)
    out = np.rint(_clip255(top + ay * (bot - top)))
    assert out.dtype == F
    return out.astype(np.uint8)


def view_batch(frames_u8, records):
    return np.stack([view_one(f, v) for f, v in zip(frames_u8, records)])


def augment_view_batch(frames_u8, params, weather, view):
    """what cilrs_augment_view_u8 must give: (uint8 [B,H,W,3], normalised float32 [B,H,W,3]);
    weather may be None"""
    shown = view_batch(frames_u8, view)
    if weather is not None:
        shown = WX.weather_batch(shown, weather)
    return AO.augment_batch(shown, WX.aug_recs(params))


def correct_steer(targets, view):
    """float32 [n, 3]: steer + steer_delta in float32, clipped to [-1, 1], where the record is on;
    written per element, independently of data.correct_steer"""
    out = np.array(targets, dtype=F, copy=True)
    for i, v in enumerate(view):
        if int(v["on"]):
            s = F(out[i, 0]) + F(v["steer_delta"])
            out[i, 0] = min(max(s, F(-1)), F(1))
    return out


def translation(dx, dy, n=1, on=1):
    """records whose two maps are source = destination + (dx, dy)"""
    from cilrs_mi355 import data as D
    v = D.identity_view(n)
    v["on"] = on
    for name in ("far", "ground"):
        v[name][:, 2], v[name][:, 5] = dx, dy
    return v


# ---- float64 pinhole camera, independent of data.view_records ------------------------------------
def intrinsics(H, W, fov_deg=100.0, w0=800, h0=600):
    f0 = (w0 / 2.0) / np.tan(np.radians(fov_deg / 2.0))
    return f0 * W / w0, f0 * H / h0, (W - 1) / 2.0, (H - 1) / 2.0


def project(X, H, W, lateral_m=0.0, yaw_rad=0.0, at_infinity=False):
    """X float64 [n, 3] in the recording camera's coordinates (x right, y down, z forward) -> pixel
    (px, py) float64 [n] in a camera moved `lateral_m` to the right and yawed `yaw_rad` to the
    right.  at_infinity: X are directions; the camera's position does not matter."""
    fx, fy, cx, cy = intrinsics(H, W)
    right = np.array([np.cos(yaw_rad), 0.0, -np.sin(yaw_rad)])
    down = np.array([0.0, 1.0, 0.0])
    fwd = np.array([np.sin(yaw_rad), 0.0, np.cos(yaw_rad)])
    rel = np.asarray(X, dtype=np.float64)
    if not at_infinity:
        rel = rel - np.array([lateral_m, 0.0, 0.0])
    xc, yc, zc = rel @ right, rel @ down, rel @ fwd
    assert (zc > 0).all(), "point behind the camera"
    return fx * xc / zc + cx, fy * yc / zc + cy


def apply_map(m9, px, py):
    """a record's 3x3 map (its float32 entries, float64 arithmetic) on pixels -> (sx, sy)"""
    m = np.asarray(m9, dtype=np.float64)
    w = m[6] * px + m[7] * py + m[8]
    return (m[0] * px + m[1] * py + m[2]) / w, (m[3] * px + m[4] * py + m[5]) / w
