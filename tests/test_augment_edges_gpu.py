"""csrc/augment.hip at the colours, shapes and borders where it can go wrong: the whole RGB cube,
shift sweeps over every tie pattern of the HSV conversion, all 256 levels of the brightness LUT,
two-pixel and odd geometry through four entry points, reads that must stay inside a sample's
frame, dropout holes, noise keys, and either output alone.  Every case compares HIP with
oracle/augment_oracle.py, which tests/test_augment_edges_host.py pins to float64 statements."""
import ctypes as C

import numpy as np
import pytest
import torch

import _augment as A
import augment_oracle as AO

pytestmark = pytest.mark.gpu


def _run(frames, p, **kw):
    """D.augment_u8 on numpy frames -> (uint8 [B,H,W,3], float32 [B,H,W,3]) as numpy."""
    from cilrs_mi355 import data as D
    t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).cuda()
    img, out8 = D.augment_u8(t, p, want_u8=True, **kw)
    return out8.cpu().numpy(), img.permute(0, 2, 3, 1).cpu().numpy()


def _dataset(cache):
    from cilrs_mi355 import data as D
    n = cache.size(0)
    return D.DeviceDataset.from_tensors(
        cache, torch.arange(n, dtype=torch.float32, device="cuda"),
        torch.arange(n, dtype=torch.int64, device="cuda"),
        torch.zeros(n, 3, dtype=torch.float32, device="cuda"))


def _assemble(cache, index, p):
    """DeviceDataset.assemble on a device cache -> (uint8, float32) as numpy; labels checked."""
    img, spd, cmd, _, out8 = _dataset(cache).assemble(np.asarray(index), p, want_u8=True)
    assert spd.cpu().tolist() == [float(i) for i in index] and cmd.cpu().tolist() == list(index)
    return out8.cpu().numpy(), img.permute(0, 2, 3, 1).cpu().numpy()


# ---- 1. the whole colour cube --------------------------------------------------------------------
@pytest.mark.parametrize("case", ("hsv", "rbc_hsv"))
def test_whole_colour_cube_exact(case):
    from cilrs_mi355 import data as D
    cube = A.colour_lattice()[None]
    p = D.identity_params(1)
    if case == "hsv":
        p["hsv_on"], p["hue"], p["sat"], p["val"] = 1, -7.3, 14.2, -9.9
    else:
        p["rbc_on"], p["alpha"], p["beta255"] = 1, 1.17, -31.5
        p["hsv_on"], p["hue"], p["sat"], p["val"] = 1, 10, -20, 15
    got8, gotf = _run(cube, p)
    want8, wantf = AO.augment_batch(cube, A.recs(p))
    assert np.array_equal(got8, want8)
    assert np.array_equal(gotf, wantf)


# ---- 2. shift sweep over every tie pattern -------------------------------------------------------
def _sweep_shifts():
    out = []
    for h in A.HUE_SWEEP:
        out += [(h, 0.0, 0.0), (h, 20.0, -15.0)]
    for s in A.SAT_SWEEP:
        out += [(0.0, s, 0.0), (10.0, s, -15.0)]
    for v in A.VAL_SWEEP:
        out += [(0.0, 0.0, v), (10.0, 20.0, v)]
    return out


def test_shift_sweep_on_the_sublattice_exact():
    """One sample per (hue, sat, val) record.  The 205,379 triples and the pixel (255, 43, 0), whose
    H = 5 a hue of nextafter(-5, -6) wraps to the last bucket, fill one [1141,180,3] frame (the
    kernel takes no one-pixel-wide frame; the colour stages do not look at geometry)."""
    from cilrs_mi355 import data as D
    sub = A.colour_sublattice()
    assert sub.shape == (205379, 1, 3)
    frame = np.concatenate([sub.reshape(-1, 3), [[255, 43, 0]]]).astype(np.uint8)
    frame = frame.reshape(1141, 180, 3)
    shifts = _sweep_shifts()
    B = len(shifts)
    p = D.identity_params(B)
    p["hsv_on"] = 1
    for b, (h, s, v) in enumerate(shifts):
        p["hue"][b], p["sat"][b], p["val"][b] = h, s, v
    frames = np.broadcast_to(frame, (B,) + frame.shape)
    got8, gotf = _run(np.ascontiguousarray(frames), p)
    want8 = np.stack([AO.augment_one(frame, r) for r in A.recs(p)])
    for b in range(B):
        assert np.array_equal(got8[b], want8[b]), shifts[b]
    assert np.array_equal(gotf, AO.normalize(want8))
    wrap = [b for b, (h, s, v) in enumerate(shifts) if h == A.HUE_SWEEP[3]]
    assert len(wrap) == 2
    for b in wrap:
        px = got8[b].reshape(-1, 3)[-1]
        assert px[2] <= 1, (shifts[b], px)           # red / orange, never (255, 0, 255)


# ---- 3. brightness / contrast at every level -----------------------------------------------------
def test_brightness_contrast_all_levels():
    from cilrs_mi355 import data as D
    ab = [(a, b) for a in (0, 0.8, 1, 1.2, 2.5) for b in (-300, -51, -0.5, 0, 0.5, 51, 300)]
    B = len(ab)
    level = np.arange(256, dtype=np.uint8).reshape(2, 128)
    frames = np.ascontiguousarray(np.broadcast_to(level[None, :, :, None], (B, 2, 128, 3)))
    p = D.identity_params(B)
    p["rbc_on"] = 1
    p["alpha"], p["beta255"] = [a for a, _ in ab], [b for _, b in ab]
    got8, gotf = _run(frames, p)
    want8, wantf = AO.augment_batch(frames, A.recs(p))
    assert np.array_equal(got8, want8) and np.array_equal(gotf, wantf)
    c = level.astype(np.float64)[None, :, :, None]
    a64 = p["alpha"].astype(np.float64)[:, None, None, None]
    b64 = p["beta255"].astype(np.float64)[:, None, None, None]
    lut = np.trunc(np.clip(c * a64 + b64, 0, 255))
    assert np.abs(got8.astype(np.float64) - lut).max() <= 1


# ---- 4. small and odd geometry, every stage, four entry points -----------------------------------
_GEOM_INDEX = (2, 0, 2, 1, 0, 2, 1)


def _geometry_params(H, W):
    from cilrs_mi355 import data as D
    p = D.identity_params(7)
    p["rbc_on"][1], p["alpha"][1], p["beta255"][1] = 1, 1.17, -31.5
    p["hsv_on"][2], p["hue"][2], p["sat"][2], p["val"][2] = 1, -7.3, 14.2, -9.9
    p["blur_k"][3], p["blur_w"][3] = 3, D.gaussian_taps(3, 0.9)
    p["blur_k"][4], p["blur_w"][4] = 5, D.gaussian_taps(5, 1.1)
    p["noise_std255"][5], p["noise_seed"][5] = 10.2, 123456789
    p["rbc_on"][6], p["alpha"][6], p["beta255"][6] = 1, 0.85, 20.0
    p["hsv_on"][6], p["hue"][6], p["sat"][6], p["val"][6] = 1, 9.0, -12.0, 6.0
    p["blur_k"][6], p["blur_w"][6] = 5, D.gaussian_taps(5, 1.1)
    p["noise_std255"][6], p["noise_seed"][6] = 10.2, 987654321
    p["nholes"][6] = 2                                        # two holes clipped to the frame
    p["hole_y0"][6, :2], p["hole_x0"][6, :2] = (0, H // 2), (0, W - 1)
    p["hole_y1"][6, :2], p["hole_x1"][6, :2] = (min(H, 1), H), (min(W, 2), W)
    return p


_geometry_cache = {}


def _geometry_case(H, W):
    """(cache [3,H,W,3], frames = cache[index], params, oracle uint8) -- computed once a shape."""
    if (H, W) not in _geometry_cache:
        assert (7 * H * W) % 256 != 0
        rng = np.random.default_rng(100 * H + W)
        cache = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        frames = np.ascontiguousarray(cache[list(_GEOM_INDEX)])
        p = _geometry_params(H, W)
        want8, _ = AO.augment_batch(frames, A.recs(p))
        want8.setflags(write=False)
        _geometry_cache[(H, W)] = (cache, frames, p, want8)
    return _geometry_cache[(H, W)]


@pytest.mark.parametrize("entry", ("augment_u8", "batch_assemble", "weather_off", "view_off"))
@pytest.mark.parametrize("H,W", A.EDGE_SHAPES)
def test_small_and_odd_geometry_every_stage(H, W, entry):
    from cilrs_mi355 import data as D
    cache, frames, p, want8 = _geometry_case(H, W)
    if entry == "augment_u8":
        got8, gotf = _run(frames, p)
    elif entry == "batch_assemble":
        got8, gotf = _assemble(torch.from_numpy(cache).cuda(), _GEOM_INDEX, p)
    elif entry == "weather_off":
        got8, gotf = _run(frames, p, weather=D.identity_weather(7))
    else:
        got8, gotf = _run(frames, p, view=D.identity_view(7))
    for b in range(7):
        d = np.abs(got8[b].astype(int) - want8[b].astype(int))
        if p["noise_std255"][b] > 0:
            assert d.max() <= 1, (b, int(d.max()))           # logf / cosf within an ulp of numpy's
        else:
            assert d.max() == 0, (b, int(d.max()))
            assert np.array_equal(gotf[b], AO.normalize(want8[b])), b
    assert np.array_equal(gotf, AO.normalize(got8))          # the float output is the bytes' own


# ---- 5. no byte outside a sample's frame is read -------------------------------------------------
@pytest.mark.parametrize("k", (5, 3))
@pytest.mark.parametrize("H,W", ((2, 2), (2, 9), (9, 2), (3, 3)))
def test_blur_reads_stay_inside_the_sample(H, W, k):
    """A tap that leaves the frame reads the neighbouring sample's row (or, for the first and last
    sample, the island's frames in front of and behind the batch): all of them hold 255 where the
    sample holds 0, and a blur of zeros is zero."""
    from cilrs_mi355 import data as D
    p = D.identity_params(3)
    p["blur_k"], p["blur_w"] = k, D.gaussian_taps(k, 1.1)
    zeros = np.zeros((3, H, W, 3), np.uint8)
    isl = A.island(zeros, 255)
    big = isl._base
    assert big.shape[0] == 5 and int(big[0].min()) == 255 and int(big[4].min()) == 255
    got8, gotf = _run(isl, p)
    assert not got8.any() and np.array_equal(gotf, AO.normalize(got8))
    got8, _ = _assemble(big, (1, 2, 3), p)
    assert not got8.any()
    mid = zeros.copy()
    mid[0] = mid[2] = 255
    isl = A.island(mid, 255)
    got8, _ = _run(isl, p)
    assert not got8[1].any() and (got8[0] == 255).all() and (got8[2] == 255).all()
    got8, _ = _assemble(isl._base, (2, 2, 2), p)
    assert not got8.any()


# ---- 6. holes -------------------------------------------------------------------------------------
def test_holes_overlap_cover_vanish_and_ignore_dead_slots():
    from cilrs_mi355 import data as D
    H, W = 12, 20
    cases = [                                  # (nholes, [(y0, x0, y1, x1)] * 3)
        (2, [(2, 3, 8, 12), (5, 8, 10, 18), (0, 0, 0, 0)]),             # overlapping
        (1, [(0, 0, H, W), (0, 0, 0, 0), (0, 0, 0, 0)]),                # the whole frame
        (1, [(4, 3, 4, 10), (0, 0, 0, 0), (0, 0, 0, 0)]),               # empty: y0 == y1
        (3, [(0, 0, 1, 1), (0, W - 1, 1, W), (H - 1, 0, H, 1)]),        # 1x1 corners
        (1, [(H - 1, W - 1, H, W), (0, 0, 0, 0), (0, 0, 0, 0)]),        # the fourth corner
        (3, [(1, 1, 3, 4), (6, 10, 11, 13), (4, 15, 9, 20)]),           # three distinct
        (1, [(3, 4, 6, 9), (0, 0, H, W), (0, 0, H, W)]),                # dead slots hold full frames
    ]
    B = len(cases)
    frames = np.random.default_rng(6).integers(1, 256, (B, H, W, 3), dtype=np.uint8)
    p = D.identity_params(B)
    live = np.zeros((B, H, W), bool)
    for b, (nh, rects) in enumerate(cases):
        p["nholes"][b] = nh
        for k, (y0, x0, y1, x1) in enumerate(rects):
            p["hole_y0"][b, k], p["hole_x0"][b, k] = y0, x0
            p["hole_y1"][b, k], p["hole_x1"][b, k] = y1, x1
            if k < nh:
                live[b, y0:y1, x0:x1] = True
    assert live[1].all() and not live[2].any() and live[3].sum() == 3 and live[6].sum() == 15
    got8, gotf = _run(frames, p)
    want8, wantf = AO.augment_batch(frames, A.recs(p))
    assert np.array_equal(got8, want8) and np.array_equal(gotf, wantf)
    assert np.array_equal(got8, np.where(live[..., None], 0, frames))   # the source has no zero


# ---- 7. noise keys --------------------------------------------------------------------------------
def test_noise_keys_and_repeated_seed():
    """Seeds at both ends of the 64-bit range.  The oracle differs from float64 Box-Muller in at
    most 1.9e-5 of the elements (host test), so a device logf / cosf within an ulp stays two orders
    of magnitude inside the cap test_augment_noise_and_random_compose already uses."""
    from cilrs_mi355 import data as D
    keys = [(s, g) for s in A.NOISE_SEEDS for g in A.NOISE_SIGMAS]
    keys += [keys[4], (2 ** 64 - 1, 15.3)]                   # seeds seen twice in one batch
    B = len(keys)
    frame = np.random.default_rng(7).integers(0, 256, (88, 200, 3), dtype=np.uint8)
    frames = np.ascontiguousarray(np.broadcast_to(frame, (B, 88, 200, 3)))
    p = D.identity_params(B)
    for b, (s, g) in enumerate(keys):
        p["noise_seed"][b], p["noise_std255"][b] = np.uint64(s), g
    got8, gotf = _run(frames, p)
    want8, _ = AO.augment_batch(frames, A.recs(p))
    diff = np.abs(got8.astype(int) - want8.astype(int))
    share = [(diff[b] > 0).mean() for b in range(B)]
    print(f"noise: max |diff| {diff.max()}, largest differing share {max(share):.3e}")
    assert diff.max() <= 1
    for b in range(B):
        assert share[b] <= 2e-3, (keys[b], share[b])
    assert np.array_equal(gotf, AO.normalize(got8))
    assert np.array_equal(got8[12], got8[4]) and np.array_equal(got8[13], got8[10])
    assert not np.array_equal(got8[0], got8[3])              # another seed, another field


# ---- 8. either output alone, through the C ABI ----------------------------------------------------
def test_either_output_alone_through_the_c_abi():
    from cilrs_mi355 import _lib as L
    from cilrs_mi355 import data as D
    B, H, W = 3, 7, 9
    frames = torch.from_numpy(
        np.random.default_rng(8).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    p = D.identity_params(B)
    p["rbc_on"][0], p["alpha"][0], p["beta255"][0] = 1, 1.17, -31.5
    p["hsv_on"][0], p["hue"][0] = 1, 9.0
    p["blur_k"][1], p["blur_w"][1] = 5, D.gaussian_taps(5, 1.1)
    p["noise_std255"][2], p["noise_seed"][2] = 10.2, 5
    p["nholes"][2] = 1
    p["hole_y0"][2, 0], p["hole_x0"][2, 0], p["hole_y1"][2, 0], p["hole_x1"][2, 0] = 1, 2, 4, 7
    pdev = torch.from_numpy(p.view(np.uint8).reshape(B, D.AUG_DTYPE.itemsize)).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(want_f, want_8):
        of = torch.full((B, H, W, 3), float("nan"), device="cuda") if want_f else None
        o8 = torch.full((B, H, W, 3), 7, dtype=torch.uint8, device="cuda") if want_8 else None
        L.check(L.lib().cilrs_augment_u8(L.ptr(frames), L.ptr(pdev), B, H, W, L.ptr(of), L.ptr(o8),
                                         stream))
        torch.cuda.synchronize()
        return of, o8

    both_f, both_8 = call(True, True)
    assert not torch.isnan(both_f).any()
    _, only_8 = call(False, True)
    only_f, _ = call(True, False)
    assert torch.equal(only_8, both_8)
    assert torch.equal(only_f.view(torch.int32), both_f.view(torch.int32))
