"""Independent float64 statements of the augmentation stages, and the frames the edge tests run on
(TEST INFRASTRUCTURE ONLY).

oracle/augment_oracle.py restates csrc/augment.hip operation for operation in float32, so a defect
the two share is invisible to a comparison between them.  The functions here state the same
operations differently -- a LUT, scipy's separable correlation with its own border, Box-Muller in
float64 -- and the host tests pin the oracle to them within the one rounding that float32 costs.
"""
import numpy as np

import augment_oracle as AO

# the levels of colour_sublattice(): every fifth level, both ends and the middle with neighbours
SUB_LEVELS = np.array(sorted(set(range(0, 256, 5)) | {1, 2, 127, 128, 129, 253, 254}), np.uint8)

# test 2 of test_augment_edges_gpu.py and the hue LUT host test share these
HUE_SWEEP = (-360.0, -180.5, -10.0, float(np.nextafter(np.float32(-5), np.float32(-6))), -0.5, 0.0,
             0.49, 10.0, 179.5, 360.0)
SAT_SWEEP = (-255.0, -20.0, 0.0, 20.0, 255.0)
VAL_SWEEP = (-255.0, -15.0, 0.0, 15.0, 255.0)

# small and odd geometry: B*H*W is a multiple of 256 at none of them for B = 7
EDGE_SHAPES = ((2, 2), (2, 3), (3, 2), (2, 7), (3, 3), (4, 5), (5, 4), (7, 9), (16, 33), (31, 17))

NOISE_SEEDS = (0, 1, 2 ** 63 - 1, 2 ** 64 - 1)
NOISE_SIGMAS = (5.1, 15.3, 80.0)


def hue_lut64(hue):
    """The hue LUT as documented: shifted half-degree hue of every H in 0..179, float64 [180]."""
    return np.trunc(np.mod(np.arange(180, dtype=np.float64) + np.float64(np.float32(hue)), 180.0))


def blur64(frame, k, sigma):
    """Gaussian blur of a uint8-valued [H,W,3] frame in float64: normalised taps exp(-x^2/2s^2),
    correlated along both axes with scipy's "mirror" border (period 2(n-1)), rounded to a level."""
    from scipy.ndimage import correlate1d
    r = k // 2
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    w /= w.sum()
    f = np.asarray(frame, dtype=np.float64)
    f = correlate1d(f, w, axis=1, mode="mirror")
    f = correlate1d(f, w, axis=0, mode="mirror")
    return np.rint(np.clip(f, 0.0, 255.0))


def noise64(seed, n):
    """Standard normal samples from the oracle's hash and bit fields, Box-Muller in float64."""
    with np.errstate(over="ignore"):
        e = np.arange(n, dtype=np.uint64)
        h = AO._splitmix64(np.uint64(seed) + e * np.uint64(0xD1B54A32D192ED03))
    u1 = ((h >> np.uint64(40)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noisy64(frame, seed, sigma255):
    """GaussNoise of a uint8 [H,W,3] frame with noise64 and the stored (float32) sigma."""
    h, w = frame.shape[:2]
    n = noise64(seed, h * w * 3).reshape(h, w, 3)
    return np.rint(np.clip(frame.astype(np.float64) + n * np.float64(np.float32(sigma255)), 0, 255))


def _lattice(levels):
    r, g, b = np.meshgrid(levels, levels, levels, indexing="ij")
    return np.stack([r, g, b], axis=-1)


def colour_lattice():
    """Every one of the 2^24 RGB triples once, as one uint8 [4096,4096,3] frame."""
    return np.ascontiguousarray(_lattice(np.arange(256, dtype=np.uint8)).reshape(4096, 4096, 3))


def colour_sublattice():
    """The 59^3 = 205,379 triples over SUB_LEVELS, uint8 [205379,1,3]: every tie pattern of the HSV
    conversion (r == g == b, two equal maxima, v == 0, d == 0) at a size a sweep can afford."""
    return np.ascontiguousarray(_lattice(SUB_LEVELS).reshape(-1, 1, 3))


def island(frames, fill):
    """frames uint8 [B,H,W,3] (numpy) -> the batch on the device as the contiguous slice
    big[1:1+B] of a tensor big [B+2,H,W,3] whose first and last frames hold `fill`: every byte one
    frame in front of and behind the batch belongs to the test and has a known value.  `big` is the
    result's `_base`."""
    import torch
    f = torch.from_numpy(np.ascontiguousarray(frames))
    b = f.size(0)
    big = torch.full((b + 2,) + tuple(f.shape[1:]), int(fill), dtype=torch.uint8, device="cuda")
    big[1:1 + b] = f.cuda()
    sl = big[1:1 + b]
    assert sl.is_contiguous() and sl._base is big
    return sl


def recs(p):
    """AUG_DTYPE records -> the list of dicts the oracle takes."""
    return [{k: (r[k].tolist() if hasattr(r[k], "tolist") else r[k]) for k in p.dtype.names}
            for r in p]


def rec(**kw):
    """One identity record as the oracle's dict, with fields replaced."""
    from cilrs_mi355 import data as D
    r = recs(D.identity_params(1))[0]
    r.update(kw)
    return r
