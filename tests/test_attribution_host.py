"""Host side of Predictor.attribution: what needs no GPU -- the C-ABI entries of
csrc/attribution.hip are declared, bound and exported, the call's own arguments are validated on
the host, and the numpy restatement of the sample batch (which tests/test_attribution_gpu.py
imports and compares the kernel against) has the statistics of a standard normal."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("cilrs_attr_samples", "cilrs_attr_accumulate", "cilrs_attr_finalize")
SMOOTHGRAD, INTEGRATED = 0, 1
IMG_MEAN = (0.485, 0.456, 0.406)
IMG_STD = (0.229, 0.224, 0.225)
TWO_PI_F32 = np.float32(6.2831853071795864)
_M64 = (1 << 64) - 1


# ---- numpy restatement of cilrs_attr_samples ------------------------------------------------------
def splitmix64(x):
    """augment.hip's hash on a uint64 array (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def sample_hash(seed, B, H, W, S, sample_ids):
    """uint64 [B, len(sample_ids), H, W, 3]: the hash word of every element,
    counter = (b*S + s)*3HW + (y*W + x)*3 + k"""
    per = 3 * H * W
    elem = np.arange(per, dtype=np.uint64).reshape(1, 1, H, W, 3)
    rows = np.array([[((b * S + s) * per) & _M64 for s in sample_ids] for b in range(B)],
                    dtype=np.uint64).reshape(B, len(sample_ids), 1, 1, 1)
    with np.errstate(over="ignore"):
        counter = rows + elem
        return splitmix64(np.uint64(seed & _M64) + counter * np.uint64(0xD1B54A32D192ED03))


def hash_normal(hsh, dtype):
    """Box-Muller on the two 24-bit fields of the hash word, every operation in `dtype` (float32:
    the kernel's formula operation by operation; float64: the same formula, same constants)"""
    u1 = ((hsh >> np.uint64(40)).astype(dtype) + dtype(1.0)) * dtype(1.0 / 16777216.0)
    u2 = ((hsh >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(dtype) * dtype(1.0 / 16777216.0)
    rad = np.sqrt(dtype(-2.0) * np.log(u1))
    return rad * np.cos(dtype(TWO_PI_F32) * u2)


def alpha_of(s, S):
    """the midpoint rule's path position of sample s of S, in float32"""
    return (np.float32(s) + np.float32(0.5)) / np.float32(S)


def samples_ref(frames, baseline, mode, S, s_begin, s_count, sigma255, seed, dtype=np.float32):
    """cilrs_attr_samples in numpy: uint8 [B,H,W,3] -> `dtype` [B*s_count,3,H,W], frame-major."""
    B, H, W, _ = frames.shape
    ids = list(range(s_begin, s_begin + s_count))
    c = frames.astype(dtype)[:, None]                                  # [B,1,H,W,3]
    if mode == INTEGRATED:
        c0 = np.zeros_like(c) if baseline is None else baseline.astype(dtype)[:, None]
        alpha = np.array([alpha_of(s, S) for s in ids], dtype=np.float32).astype(dtype)
        v = c0 + alpha.reshape(1, -1, 1, 1, 1) * (c - c0)
    else:
        n = hash_normal(sample_hash(seed, B, H, W, S, ids), dtype)
        v = c + dtype(np.float32(sigma255)) * n
    m = np.array(IMG_MEAN, dtype=np.float32).astype(dtype)
    d = np.array(IMG_STD, dtype=np.float32).astype(dtype)
    out = (v / dtype(255.0) - m) / d                                   # [B,n,H,W,3]
    assert out.dtype == dtype
    return np.ascontiguousarray(out.transpose(0, 1, 4, 2, 3)).reshape(B * s_count, 3, H, W)


# ---- the tests ----------------------------------------------------------------------------------------
def test_attribution_entries_are_declared_bound_and_exported():
    from cilrs_mi355 import _lib as L
    header = open(os.path.join(ROOT, "include", "cilrs_hip.h")).read()
    lib = L.lib()
    for name in NEW_ENTRIES + ("cilrs_attr_finalize_threads",):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in L.SIGNATURES
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert re.search(r"#define CILRS_ATTR_SMOOTHGRAD %d\b" % SMOOTHGRAD, header)
    assert re.search(r"#define CILRS_ATTR_INTEGRATED %d\b" % INTEGRATED, header)
    threads = lib.cilrs_attr_finalize_threads()
    assert threads >= 64 and threads % 64 == 0


def test_attribution_argument_validation():
    from cilrs_mi355.predict import Predictor
    chk = Predictor._attribution_args
    shape = (2, 88, 200, 3)
    assert Predictor.ATTRIBUTION_METHODS == {"smoothgrad": SMOOTHGRAD, "integrated": INTEGRATED}
    dflt = Predictor.ATTRIBUTION_CHUNK
    assert dflt in (8, 16, 32)
    assert chk("smoothgrad", 32, 0.15, None, 0, None, shape) == (SMOOTHGRAD, 32, 255.0 * 0.15, None, 0,
                                                                 min(32, dflt))
    assert chk("smoothgrad", 3, 0, None, 7, None, shape) == (SMOOTHGRAD, 3, 0.0, None, 7, 3)
    assert chk("smoothgrad", 5, 0.1, None, 2 ** 64 - 1, 64, shape)[4:] == (2 ** 64 - 1, 5)
    assert chk("integrated", np.int64(9), 0.15, None, 0, 4, shape)[:2] == (INTEGRATED, 9)
    base = np.zeros(shape, dtype=np.uint8)
    assert chk("integrated", 4, 0.15, base, 0, 3, shape)[3] is base
    for bad in (dict(method="vargrad"), dict(method=None), dict(method=0),
                dict(samples=0), dict(samples=-3), dict(samples=2.5), dict(samples=True),
                dict(samples=None), dict(samples=1 << 24),
                dict(sigma=-0.1), dict(sigma=float("nan")), dict(sigma=float("inf")),
                dict(sigma="wide"), dict(sigma=None),
                dict(method="integrated", baseline=np.zeros((2, 88, 200), dtype=np.uint8)),
                dict(method="integrated", baseline=np.zeros((1, 88, 200, 3), dtype=np.uint8)),
                dict(method="integrated", baseline=np.zeros(shape, dtype=np.float32)),
                dict(method="smoothgrad", baseline=base),
                dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5),
                dict(chunk=0), dict(chunk=-2), dict(chunk=1.5)):
        args = dict(method="smoothgrad", samples=8, sigma=0.15, baseline=None, seed=0, chunk=None)
        args.update(bad)
        with pytest.raises(ValueError, match="attribution"):
            chk(frames_shape=shape, **args)


def test_alpha_is_the_fp32_midpoint_formula():
    for S in (1, 4, 5, 32, 1000):
        a = np.array([alpha_of(s, S) for s in range(S)])
        assert a.dtype == np.float32
        want = ((np.arange(S, dtype=np.float32) + np.float32(0.5)) / np.float32(S))
        assert np.array_equal(a, want.astype(np.float32))
        assert 0.0 < a.min() and a.max() < 1.0 and np.all(np.diff(a) > 0)
        assert abs(float(a.astype(np.float64).mean()) - 0.5) <= 1e-6       # midpoints of [0, 1]
    assert alpha_of(0, 1) == np.float32(0.5)
    # alpha = 1 is not a midpoint, but the restatement then gives the frame's own preprocessing
    f = (np.arange(2 * 3 * 5 * 3) % 256).astype(np.uint8).reshape(2, 3, 5, 3)
    ig = samples_ref(f, None, INTEGRATED, 1, 0, 1, 0.0, 0)
    assert ig.shape == (2, 3, 3, 5) and ig.dtype == np.float32


def test_sample_noise_is_a_standard_normal():
    H, W = 88, 200
    N = 3 * H * W
    for seed, s in ((0, 0), (12345, 7)):
        h = sample_hash(seed, 1, H, W, 32, [s])
        n32 = hash_normal(h, np.float32)
        assert n32.dtype == np.float32 and n32.shape == (1, 1, H, W, 3)
        assert np.isfinite(n32).all()
        n = n32.astype(np.float64).ravel()
        assert abs(n.mean()) <= 4.0 / np.sqrt(N)
        assert abs(n.var() - 1.0) <= 4.0 * np.sqrt(2.0 / N)
        # the float64 evaluation of the same bits is the same numbers to fp32 accuracy
        assert np.abs(n - hash_normal(h, np.float64).ravel()).max() <= 1e-5
    # keyed on the global sample index: a chunk is a slice of the whole, another seed is not
    whole = sample_hash(3, 2, 4, 6, 5, [0, 1, 2, 3, 4])
    assert np.array_equal(whole[:, 2:4], sample_hash(3, 2, 4, 6, 5, [2, 3]))
    assert not np.array_equal(whole, sample_hash(4, 2, 4, 6, 5, [0, 1, 2, 3, 4]))
    assert len(np.unique(whole)) == whole.size


def test_samples_restatement_without_noise_is_the_preprocessing():
    import cilrs_oracle as O
    frames = O.synthetic_batch(2, seed=5)[4]
    want = np.concatenate([O.preprocess_frame(f).numpy() for f in frames])
    got = samples_ref(frames, None, SMOOTHGRAD, 3, 0, 3, 0.0, 11)
    assert got.dtype == np.float32
    for b in range(2):
        for j in range(3):
            assert np.array_equal(got[b * 3 + j], want[b])
