"""The four kernels of csrc/adversarial.hip restated in numpy (include/cilrs_hip.h "adversarial
robustness" is the definition): fp32 operation by operation -- what the device must equal bit for
bit -- and, with dtype=np.float64, the same formulas in double for comparison.

All tensors are logical NCHW [B,3,H,W]; strides do not exist here (the draw is keyed on the logical
element index, which is the point)."""
import numpy as np

IMG_MEAN = (0.485, 0.456, 0.406)
IMG_STD = (0.229, 0.224, 0.225)
CHAN_SCALE = tuple(1.0 / (255.0 * s) for s in IMG_STD)
M64 = (1 << 64) - 1


def range6():
    """the images of the bytes 0 and 255 under the preprocessing, in its fp32 operation order"""
    out = []
    for m, d in zip(IMG_MEAN, IMG_STD):
        for byte in (0.0, 255.0):
            out.append(float((np.float32(byte) / np.float32(255.0) - np.float32(m)) / np.float32(d)))
    return tuple(out)


RANGE6 = range6()


def splitmix64(x):
    """the finaliser of csrc/common.h on uint64 arrays (wrapping arithmetic)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draw_u(seed, shape, dtype=np.float32):
    """u of every element of a [B,3,H,W] tensor: the first 24-bit field of the hash of its logical
    index, in (0, 1]"""
    n = int(np.prod(shape))
    counter = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = splitmix64(np.uint64(seed & M64) + counter * np.uint64(0xD1B54A32D192ED03))
    top = (h >> np.uint64(40)).astype(np.uint32)
    u = (top.astype(dtype) + dtype(1.0)) * dtype(1.0 / 16777216.0)
    return u.reshape(shape)


def per_channel(level, dtype=np.float32):
    """level (8-bit levels) * chan_scale3 as a [1,3,1,1] array: one product per channel.  The fp32
    form multiplies the fp32 roundings, as the C entry does; the float64 form is exact inputs."""
    if dtype == np.float32:
        v = [np.float32(level) * np.float32(s) for s in CHAN_SCALE]
    else:
        v = [np.float64(level) * np.float64(s) for s in CHAN_SCALE]
    return np.asarray(v, dtype=dtype).reshape(1, 3, 1, 1)


def clamp(t, x, e, rng, dtype=np.float32):
    t = np.fmin(np.fmax(t, x - e), x + e)
    if rng is not None:
        lo = np.asarray(rng[0::2], dtype=dtype).reshape(1, 3, 1, 1)
        hi = np.asarray(rng[1::2], dtype=dtype).reshape(1, 3, 1, 1)
        t = np.fmin(np.fmax(t, lo), hi)
    return t


def start_ref(x, eps255, seed, rng=None, dtype=np.float32):
    x = np.asarray(x, dtype=dtype)
    if not eps255 > 0:
        return x.copy()
    e = per_channel(eps255, dtype)
    u = draw_u(seed, x.shape, dtype)
    r = (u + u) - dtype(1.0)
    return clamp(x + e * r, x, e, rng, dtype).astype(dtype)


def step_ref(x, x_adv, g, alpha255, eps255, row_dir=None, improved=None, best=None, rng=None,
             dtype=np.float32):
    """-> (x_adv after, best after); best None stays None"""
    x, x_adv = np.asarray(x, dtype=dtype), np.asarray(x_adv, dtype=dtype)
    if improved is not None and best is not None:
        best = np.where(np.asarray(improved).reshape(-1, 1, 1, 1) != 0, x_adv, best).astype(dtype)
    if not alpha255 > 0:
        return x_adv.copy(), best
    g = np.asarray(g, dtype=dtype)
    s = np.where(g > 0, dtype(1.0), np.where(g < 0, dtype(-1.0), dtype(0.0))).astype(dtype)
    a = per_channel(alpha255, dtype)
    d = np.ones((x.shape[0], 1, 1, 1), dtype=dtype) if row_dir is None else \
        np.asarray(row_dir, dtype=dtype).reshape(-1, 1, 1, 1)
    with np.errstate(invalid="ignore"):
        t = x_adv + (a * d) * s
    return clamp(t, x, per_channel(eps255, dtype), rng, dtype).astype(dtype), best


def direction_ref(controls, pred_speed, ref_controls, ref_speed, w4, first, best_dev,
                  dtype=np.float32):
    """-> (dev, best_dev after, row_dir, improved)"""
    c, r = np.asarray(controls, dtype=dtype), np.asarray(ref_controls, dtype=dtype)
    s, rs = np.asarray(pred_speed, dtype=dtype), np.asarray(ref_speed, dtype=dtype)
    w = [dtype(v) for v in w4]
    with np.errstate(invalid="ignore", over="ignore"):
        dev = (w[0] * (c[:, 0] - r[:, 0]) + w[1] * (c[:, 1] - r[:, 1])) + \
              (w[2] * (c[:, 2] - r[:, 2]) + w[3] * (s - rs))
        dev = dev.astype(dtype)
        finite = np.isfinite(dev)
        row_dir = np.where(~finite | (dev >= 0), dtype(1.0), dtype(-1.0)).astype(dtype)
        if first:
            improved = finite.copy()
            best = np.where(finite, dev, dtype(0.0)).astype(dtype)
        else:
            best_dev = np.asarray(best_dev, dtype=dtype)
            improved = finite & (np.abs(dev) > np.abs(best_dev))
            best = np.where(improved, dev, best_dev).astype(dtype)
    return dev, best, row_dir, improved.astype(np.int32)


def quantize_ref(x_adv, frames_u8=None, dtype=np.float32):
    """-> (uint8 [B,H,W,3], linf int32 [B] or None)"""
    x_adv = np.asarray(x_adv, dtype=dtype)
    d = np.asarray(IMG_STD, dtype=dtype).reshape(1, 3, 1, 1)
    m = np.asarray(IMG_MEAN, dtype=dtype).reshape(1, 3, 1, 1)
    with np.errstate(invalid="ignore"):
        v = (x_adv * d + m) * dtype(255.0)
        v = np.fmin(np.fmax(v, dtype(0.0)), dtype(255.0))
    q = np.rint(v).astype(np.uint8).transpose(0, 2, 3, 1).copy()
    linf = None
    if frames_u8 is not None:
        diff = np.abs(q.astype(np.int32) - np.asarray(frames_u8).astype(np.int32))
        linf = diff.reshape(diff.shape[0], -1).max(1).astype(np.int32)
    return q, linf


def preprocess(frames_u8, dtype=np.float32):
    """uint8 [B,H,W,3] -> the network input [B,3,H,W]: (c / 255 - mean) / std in that order"""
    c = np.asarray(frames_u8).astype(dtype).transpose(0, 3, 1, 2)
    m = np.asarray(IMG_MEAN, dtype=dtype).reshape(1, 3, 1, 1)
    d = np.asarray(IMG_STD, dtype=dtype).reshape(1, 3, 1, 1)
    return ((c / dtype(255.0) - m) / d).astype(dtype)
