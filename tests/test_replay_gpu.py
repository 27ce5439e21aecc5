"""Closed-loop replay on the device: `cilrs_replay_begin` / `_step` / `_finish` against the float64
definition in tests/_replay.py on crafted controls (inside guard bands, permuted, twice), and
`evaluate.replay` end to end, teacher-forced: every traced tick must follow from the previous traced
tick by the definition, and every tick's controls must be the model's on the frames assembled from
that tick's traced records -- chaos in the loop cannot hide anything this way."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _replay as RP
import cilrs_oracle as O
from _guards import Inputs, guarded

pytestmark = pytest.mark.gpu

H, W, N = 88, 200, 40
T_OP = 8
TAPS = (1.0, 2.0, 3.0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def dataset():
    """40 random frames; frames 0..8 stand still, the rest drive at 0.2 .. 1 of 40 km/h; frames
    22..35 share the label 0.125, whose weighted mean under any taps used here is 0.125 exactly"""
    from cilrs_mi355 import data as D
    g = torch.Generator().manual_seed(11)
    cache = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)
    speed = 0.2 + 0.8 * torch.rand(N, generator=g)
    speed[:9] = 0.0
    command = torch.randint(0, 4, (N,), generator=g)
    targets = torch.rand(N, 3, generator=g)
    targets[:, 0] = 0.3 * (targets[:, 0] * 2 - 1)
    targets[20, 0], targets[21, 0] = 1.5, -1.5               # labels beyond the lock: clipped
    targets[22:36, 0] = 0.125
    return D.DeviceDataset.from_tensors(cache.cuda(), speed.cuda(), command.cuda(), targets.cuda())


# name, start frame, lateral0 [m], yaw0 [deg], raw steer of tick k given the clipped label
NAN, INF = float("nan"), float("inf")
CASES = (
    ("lateral limit", 23, 0.97, 3.0, lambda k, sx: sx),
    ("yaw limit", 12, 0.0, 9.0, lambda k, sx: sx + 0.2),
    ("exactly at the limit", 22, 1.0, 0.0, lambda k, sx: sx),
    ("NaN steer", 16, 0.3, 1.0, lambda k, sx: NAN if k in (2, 7) else 0.1),
    ("inf steer", 18, -0.3, -1.0, lambda k, sx: INF if k == 3 else (-INF if k == 5 else -0.1)),
    ("steer +-3", 20, 0.1, 0.5, lambda k, sx: 3.0 if k % 2 == 0 else -3.0),
    ("speed 0", 0, 0.4, -3.0, lambda k, sx: 0.5),
    ("zero state", 26, 0.0, 0.0, lambda k, sx: sx),
    ("filtered", 30, -0.5, -2.0, lambda k, sx: 0.05 * math.sin(1.7 * k) + sx),
)


def _crafted(ds, B):
    """B segments cycling through CASES (the first is case B % 9, so B = 1 and B = 5 reach
    different ones) with their controls [T, B, 3] float32"""
    speed = ds.speed.cpu().numpy()
    targets = ds.targets.cpu().numpy()
    which = [(b + B) % len(CASES) for b in range(B)]
    # every second round of the cases starts one frame later: other speeds and labels
    start = np.array([CASES[c][1] + (b // len(CASES)) % 2 for b, c in enumerate(which)],
                     dtype=np.int64)
    lat0 = np.array([CASES[c][2] for c in which], dtype=np.float64)
    yaw0 = np.radians(np.array([CASES[c][3] for c in which], dtype=np.float64))
    controls = np.zeros((T_OP, B, 3), dtype=np.float32)
    for b, c in enumerate(which):
        for k in range(T_OP):
            sx = RP.clip1(float(targets[start[b] + k, 0]))
            controls[k, b, 0] = CASES[c][4](k, sx)
    controls[:, :, 1:] = 0.25
    return which, start, lat0, yaw0, controls, speed, targets


def _config(taps, closed_loop=True, max_yaw_deg=10.0):
    from cilrs_mi355 import _lib as L
    from cilrs_mi355 import data as D
    fx, fy, cx, cy = D.CameraModel().intrinsics(H, W)
    return L.ReplayConfig(
        dt_s=0.05, speed_unit_ms=D.SPEED_NORM_KMH / 3.6, wheelbase_m=2.875,
        max_wheel_rad=float(np.radians(70.0)), lookahead_s=1.0, min_lookahead_m=4.0, fx=fx, fy=fy,
        cx=cx, cy=cy, height_m=1.4, max_lateral_m=1.0, max_yaw_rad=float(np.radians(max_yaw_deg)),
        recover_m=0.1, taps=(C.c_double * 8)(*taps), ntaps=len(taps),
        closed_loop=1 if closed_loop else 0)


def _run_op(ds, cfg, start, lat0, yaw0, controls, guards=True):
    """begin, T - 1 steps and finish on crafted controls -> dict of host arrays"""
    from cilrs_mi355 import _lib as L
    from cilrs_mi355 import data as D
    lib = L.lib()
    B = len(start)
    ns, nm = lib.cilrs_replay_state_doubles(), lib.cilrs_replay_metric_doubles()
    checks = []

    def buf(shape, dtype, fill, name):
        n = int(np.prod(shape))
        if not guards:
            return torch.full((n,), fill, dtype=dtype, device="cuda").view(shape)
        t, chk = guarded(n, dtype, fill, n, name)
        checks.append(chk)
        return t.view(shape)

    nan = float("nan")
    state = buf((B, ns), torch.float64, nan, "state")
    metrics = buf((B, nm), torch.float64, nan, "metrics")
    index = buf((T_OP, B), torch.int64, -1, "index")
    view = buf((T_OP, B, D.VIEW_DTYPE.itemsize), torch.uint8, 0xEE, "view")
    tstate = buf((T_OP, B, 2), torch.float64, nan, "trace_state")
    tsteer = buf((T_OP, B, 2), torch.float32, 7.0, "trace_steer")
    tflags = buf((T_OP, B), torch.uint8, 0xEE, "trace_flags")
    cdev = torch.from_numpy(controls).cuda()
    ins = Inputs(speed=ds.speed, targets=ds.targets, controls=cdev)
    start, lat0, yaw0 = (np.ascontiguousarray(a) for a in (start, lat0, yaw0))
    vp = C.c_void_p
    L.check(lib.cilrs_replay_begin(
        C.byref(cfg), B, T_OP, N, vp(start.ctypes.data), vp(lat0.ctypes.data),
        vp(yaw0.ctypes.data), L.ptr(ds.speed), L.ptr(state), L.ptr(metrics), L.ptr(index[0]),
        L.ptr(view[0]), _stream()))
    for k in range(1, T_OP):
        L.check(lib.cilrs_replay_step(
            C.byref(cfg), B, k, L.ptr(cdev[k - 1]), L.ptr(ds.speed), L.ptr(ds.targets), N,
            L.ptr(state), L.ptr(metrics), L.ptr(index[k]), L.ptr(view[k]), L.ptr(tstate[k - 1]),
            L.ptr(tsteer[k - 1]), L.ptr(tflags[k - 1]), _stream()))
    L.check(lib.cilrs_replay_finish(
        C.byref(cfg), B, T_OP, L.ptr(cdev[T_OP - 1]), L.ptr(ds.speed), L.ptr(ds.targets), N,
        L.ptr(state), L.ptr(metrics), L.ptr(tstate[T_OP - 1]), L.ptr(tsteer[T_OP - 1]),
        L.ptr(tflags[T_OP - 1]), _stream()))
    for chk in checks:
        chk()
    ins.check()
    out = {k: t.cpu().numpy() for k, t in dict(
        state=state, metrics=metrics, index=index, tstate=tstate, tsteer=tsteer,
        tflags=tflags).items()}
    out["view"] = np.ascontiguousarray(view.cpu().numpy()).view(D.VIEW_DTYPE)[..., 0]
    return out


def _close_f32(dev, host, what):
    """one float32 rounding apart: |device - host| <= spacing(float32 |host|) + 1e-11"""
    dev64, host64 = dev.astype(np.float64), host.astype(np.float64)
    tol = np.spacing(np.abs(host.astype(np.float32))).astype(np.float64) + 1e-11
    bad = np.abs(dev64 - host64) > tol
    assert not bad.any(), (what, dev64[bad][:3], host64[bad][:3])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


COUNTS = ("ticks", "lateral_interventions", "yaw_interventions", "nonfinite", "recover_tick",
          "steer_ticks")


@pytest.mark.parametrize("B,taps", [(1, ()), (5, TAPS), (257, TAPS)])
def test_op_level_against_the_definition(dataset, B, taps):
    from cilrs_mi355 import data as D
    ds = dataset
    which, start, lat0, yaw0, controls, speed, targets = _crafted(ds, B)
    got = _run_op(ds, _config(taps), start, lat0, yaw0, controls)
    rcfg = RP.Config(steer_filter=taps, height=H, width=W)
    ident = D.identity_view(1).tobytes()
    seen = set()
    for b in range(B):
        name = CASES[which[b]][0]
        seg = RP.Segment(rcfg, lat0[b], yaw0[b])
        for k in range(T_OP):
            i = int(start[b]) + k
            tag = (name, b, k)
            assert got["index"][k, b] == i, tag
            e_d, psi_d = got["tstate"][k, b]
            assert abs(e_d - seg.e) <= 1e-12 and abs(psi_d - seg.psi) <= 1e-12, tag
            rec = got["view"][k, b:b + 1]
            if e_d == 0.0 and psi_d == 0.0:
                assert rec.tobytes() == ident, tag
                seen.add("identity")
            else:
                want = D.view_records(e_d, psi_d, float(speed[i]), H, W)
                assert rec["on"][0] == 1 and rec["reserved"][0] == 0, tag
                assert rec["split_row"][0] == want["split_row"][0], tag
                for field in ("far", "ground", "steer_delta", "lateral_m", "yaw_rad"):
                    _close_f32(rec[field], want[field], tag + (field,))
                D.check_view(rec, H, W)
            s, flags = seg.advance(float(controls[k, b, 0]), speed[i], targets[i, 0])
            assert got["tflags"][k, b] == flags, tag
            raw_d, s_d = got["tsteer"][k, b]
            np.testing.assert_array_equal(raw_d, controls[k, b, 0], err_msg=str(tag))
            np.testing.assert_array_equal(s_d, np.float32(s), err_msg=str(tag))
            if flags & ~RP.FLAG_ON:
                seen.add((name, flags & ~RP.FLAG_ON))
        # the state after the last tick, the counts exactly, the sums to 1e-12 relative
        assert abs(got["state"][b, 0] - seg.e) <= 1e-12, name
        assert abs(got["state"][b, 1] - seg.psi) <= 1e-12, name
        assert np.isfinite(got["state"][b]).all() and np.isfinite(got["metrics"][b]).all(), name
        for j, key in enumerate(RP.METRICS):
            d, h = got["metrics"][b, j], seg.m[key]
            if key in COUNTS:
                assert d == h, (name, key, d, h)
            else:
                assert abs(d - h) <= 1e-12 * abs(h), (name, key, d, h)
        if name == "exactly at the limit":
            assert seg.m["lateral_interventions"] == 0 and got["state"][b, 0] == 1.0
        if name == "speed 0":
            assert got["state"][b, 0] == lat0[b] and got["state"][b, 1] == yaw0[b]
        if name == "zero state":
            assert all(got["view"][k, b:b + 1].tobytes() == ident for k in range(T_OP))
    if B >= len(CASES):                   # every crafted case did what its name says
        assert ("lateral limit", RP.FLAG_LATERAL) in seen and ("yaw limit", RP.FLAG_YAW) in seen
        assert ("NaN steer", RP.FLAG_NONFINITE) in seen and ("inf steer", RP.FLAG_NONFINITE) in seen
        assert any(n == "steer +-3" for n, _f in seen - {"identity"}) and "identity" in seen


def test_op_level_permuted_and_twice(dataset):
    ds = dataset
    B = 67
    which, start, lat0, yaw0, controls, speed, targets = _crafted(ds, B)
    cfg = _config(TAPS)
    a = _run_op(ds, cfg, start, lat0, yaw0, controls, guards=False)
    again = _run_op(ds, cfg, start, lat0, yaw0, controls, guards=False)
    perm = np.random.default_rng(5).permutation(B)
    assert not np.array_equal(perm // 64, np.arange(B) // 64)        # segments change their wave
    p = _run_op(ds, cfg, start[perm], lat0[perm], yaw0[perm],
                np.ascontiguousarray(controls[:, perm]), guards=False)
    for key in a:
        assert _same_bits(a[key], again[key]), key
        moved = a[key][perm] if key in ("state", "metrics") else a[key][:, perm]
        assert _same_bits(np.ascontiguousarray(moved), p[key]), key


def test_begin_and_step_refuse_bad_arguments(dataset):
    from cilrs_mi355 import _lib as L
    ds = dataset
    lib = L.lib()
    ns, nm = lib.cilrs_replay_state_doubles(), lib.cilrs_replay_metric_doubles()
    state = torch.full((2, ns), 3.0, dtype=torch.float64, device="cuda")
    metrics = torch.full((2, nm), 3.0, dtype=torch.float64, device="cuda")
    index = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    view = torch.full((2, 96), 0xEE, dtype=torch.uint8, device="cuda")
    vp = C.c_void_p
    lat = np.zeros(2)

    def begin(cfg=None, B=2, ticks=4, start=(0, 3), lat0=lat, yaw0=lat, null=False):
        st = np.array(start, dtype=np.int64)
        return lib.cilrs_replay_begin(
            C.byref(cfg or _config(())), B, ticks, N, None if null else vp(st.ctypes.data),
            vp(np.ascontiguousarray(lat0).ctypes.data), vp(np.ascontiguousarray(yaw0).ctypes.data),
            L.ptr(ds.speed), L.ptr(state), L.ptr(metrics), L.ptr(index), L.ptr(view), _stream())

    nine = _config(())
    nine.ntaps = 9
    for why, kw in (("start < 0", dict(start=(0, -1))), ("past the end", dict(start=(0, N - 3))),
                    ("B < 1", dict(B=0)), ("ticks < 1", dict(ticks=0)), ("NULL", dict(null=True)),
                    ("nine taps", dict(cfg=nine)),
                    ("start outside the box", dict(lat0=np.array([0.0, 1.5]))),
                    ("NaN start", dict(yaw0=np.array([math.nan, 0.0])))):
        assert begin(**kw) != 0, why
        assert lib.cilrs_last_error(), why
    assert lib.cilrs_replay_step(C.byref(_config(())), 2, 0, L.ptr(view), L.ptr(ds.speed),
                                 L.ptr(ds.targets), N, L.ptr(state), L.ptr(metrics), L.ptr(index),
                                 L.ptr(view), None, None, None, _stream()) != 0, "tick 0"
    torch.cuda.synchronize()
    # nothing was launched: every buffer is as it was
    assert bool((state == 3.0).all()) and bool((metrics == 3.0).all())
    assert bool((index == -7).all()) and bool((view == 0xEE).all())
    assert begin(start=(0, N - 4)) == 0                           # the last frame is reachable


# ---- evaluate.replay -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from cilrs_mi355 import CILRS
    m = CILRS(4, dropout=0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0), strict=True)
    return m.cuda().eval()


B_E2E, T_E2E = 5, 6
STARTS = np.array([0, 7, 13, 22, N - T_E2E])


def _controls_of(model, ds, index, view=None, weather=None):
    from cilrs_mi355 import data as D
    img, spd, cmd, _tgt = ds.assemble(index, D.identity_params(len(index)), weather=weather,
                                      view=view)
    with torch.no_grad():
        return model(img, spd, cmd)[0]


def test_replay_teacher_forced(dataset, model):
    from cilrs_mi355 import evaluate as E
    ds = dataset
    taps = (1.0, 2.0)
    rep = E.replay(model, ds, STARTS, T_E2E, lateral_m=0.3, yaw_deg=2.0, steer_filter=taps,
                   trace=True)
    assert set(rep) == {"config", "segments", "overall", "trace"}
    tr = rep["trace"]
    assert tr["e"].shape == tr["psi"].shape == tr["flags"].shape == (T_E2E, B_E2E)
    assert tr["controls"].shape == (T_E2E, B_E2E, 3) and tr["view"].shape == (T_E2E, B_E2E)
    assert np.array_equal(tr["index"], STARTS[None, :] + np.arange(T_E2E)[:, None])
    assert (tr["e"][0] == 0.3).all() and (tr["psi"][0] == math.radians(2.0)).all()
    speed, targets = ds.speed.cpu().numpy(), ds.targets.cpu().numpy()
    rcfg = RP.Config(steer_filter=taps, height=H, width=W)
    for b in range(B_E2E):
        seg = RP.Segment(rcfg, 0.3, math.radians(2.0))
        for k in range(T_E2E):
            i = int(STARTS[b]) + k
            seg.e, seg.psi = float(tr["e"][k, b]), float(tr["psi"][k, b])      # teacher forcing
            raw = tr["raw_steer"][k, b]
            assert raw.tobytes() == tr["controls"][k, b, 0].tobytes()
            s, flags = seg.advance(float(raw), speed[i], targets[i, 0])
            assert flags == tr["flags"][k, b], (b, k)
            np.testing.assert_array_equal(tr["steer"][k, b], np.float32(s))
            if k + 1 < T_E2E:
                assert abs(seg.e - tr["e"][k + 1, b]) <= 1e-12, (b, k)
                assert abs(seg.psi - tr["psi"][k + 1, b]) <= 1e-12, (b, k)
    # the controls of every tick are the model's on that tick's traced records
    for k in range(T_E2E):
        got = torch.from_numpy(tr["controls"][k]).cuda()
        assert torch.equal(_controls_of(model, ds, tr["index"][k], view=tr["view"][k]), got), k
    assert (tr["view"]["on"][0] == 1).all()
    # the report: counts are the flags', autonomy by its formula
    for b, seg in enumerate(rep["segments"]):
        f = tr["flags"][:, b]
        assert seg["ticks"] == T_E2E and seg["start"] == STARTS[b]
        assert seg["lateral_interventions"] == int(((f & 1) != 0).sum())
        assert seg["yaw_interventions"] == int(((f & 2) != 0).sum())
        assert seg["nonfinite"] == int(((f & 4) != 0).sum()) == 0
        n = seg["lateral_interventions"] + seg["yaw_interventions"]
        assert seg["autonomy"] == max(0.0, 1.0 - 6.0 * n / (T_E2E * 0.05))
        assert seg["sum_abs_e"] == pytest.approx(np.abs(tr["e"][:, b]).sum(), rel=1e-12)
        assert seg["max_abs_psi"] == np.abs(tr["psi"][:, b]).max()
    assert rep["overall"]["ticks"] == B_E2E * T_E2E and rep["overall"]["segments"] == B_E2E
    # batches of segments: two at a time, every batch's controls are the model's at that batch
    tr = E.replay(model, ds, STARTS, T_E2E, lateral_m=0.3, yaw_deg=2.0, steer_filter=taps,
                  batch_size=2, trace=True)["trace"]
    assert np.array_equal(tr["index"], STARTS[None, :] + np.arange(T_E2E)[:, None])
    assert (tr["e"][0] == 0.3).all() and tr["controls"].shape == (T_E2E, B_E2E, 3)
    for k in range(T_E2E):
        for lo in range(0, B_E2E, 2):
            got = torch.from_numpy(tr["controls"][k, lo:lo + 2]).cuda()
            want = _controls_of(model, ds, tr["index"][k, lo:lo + 2], view=tr["view"][k, lo:lo + 2])
            assert torch.equal(want, got), (k, lo)


def test_replay_open_loop_at_zero_reads_the_stored_frames(dataset, model):
    from cilrs_mi355 import data as D
    from cilrs_mi355 import evaluate as E
    ds = dataset
    rep = E.replay(model, ds, STARTS, T_E2E, closed_loop=False, trace=True)
    tr = rep["trace"]
    assert tr["view"].tobytes() == D.identity_view(T_E2E * B_E2E).tobytes()
    assert (tr["e"] == 0).all() and (tr["psi"] == 0).all() and (tr["flags"] == 0).all()
    for k in range(T_E2E):
        got = torch.from_numpy(tr["controls"][k]).cuda()
        assert torch.equal(_controls_of(model, ds, tr["index"][k]), got), k
    assert all(s["max_abs_e"] == 0 and s["autonomy"] == 1.0 for s in rep["segments"])
    # per segment, one float per per-tick value: each start pose is the segment's own
    lat = np.array([0.0, 0.1, -0.2, 0.3, -0.4])
    rep = E.replay(model, ds, STARTS, T_E2E, lateral_m=lat, yaw_deg=-lat * 10, closed_loop=False,
                   trace=True)
    assert (rep["trace"]["e"] == lat[None, :]).all()
    assert (rep["trace"]["psi"] == np.radians(-lat * 10)[None, :]).all()
    assert [s["recover_tick"] for s in rep["segments"]] == [-1] * B_E2E


def test_replay_under_weather(dataset, model):
    from cilrs_mi355 import data as D
    from cilrs_mi355 import evaluate as E
    ds = dataset
    mix = D.WeatherMix.fixed("fog", 0.5)
    rep = E.replay(model, ds, STARTS, T_E2E, lateral_m=-0.2, yaw_deg=1.0, weather=mix, seed=3,
                   trace=True)
    tr = rep["trace"]
    wrec = mix.draw(np.random.default_rng([3, D.WEATHER_STREAM]), T_E2E * B_E2E, H, W) \
        .reshape(T_E2E, B_E2E)
    assert (wrec["fog_on"] == 1).all()
    for k in range(T_E2E):
        got = torch.from_numpy(tr["controls"][k]).cuda()
        want = _controls_of(model, ds, tr["index"][k], view=tr["view"][k], weather=wrec[k])
        assert torch.equal(want, got), k
    clear = _controls_of(model, ds, tr["index"][0], view=tr["view"][0])
    assert not torch.equal(clear, torch.from_numpy(tr["controls"][0]).cuda())
    assert rep["config"]["weather"] == {"names": ["fog"], "severity": [0.5, 0.5]}


def test_replay_refusals_and_mode(dataset, model, tmp_path):
    import json
    from cilrs_mi355 import data as D
    from cilrs_mi355 import evaluate as E
    ds = dataset
    empty = D.DeviceDataset.from_tensors(ds.cache, ds.speed, ds.command_dev, ds.targets)
    empty.cache = None
    assert not empty.filled
    for why, call in (
            ("unfilled", lambda: E.replay(model, empty, [0], 4)),
            ("start < 0", lambda: E.replay(model, ds, [0, -1], 4)),
            ("past the end", lambda: E.replay(model, ds, [0, N - 3], 4)),
            ("ticks < 1", lambda: E.replay(model, ds, [0], 0)),
            ("nine taps", lambda: E.replay(model, ds, [0], 4, steer_filter=[1.0] * 9)),
            ("yaw box too wide for the camera", lambda: E.replay(model, ds, [0], 4,
                                                                 max_yaw_deg=40.0)),
            ("start outside the box", lambda: E.replay(model, ds, [0], 4, lateral_m=1.5))):
        with pytest.raises(RuntimeError):
            call()
    # 40 degrees is refused by the corner record, not by a blanket rule: 15 degrees passes
    D.check_view(D.view_records(1.0, np.radians(15.0), 0.0, H, W), H, W)
    with pytest.raises(RuntimeError, match="w falls below"):
        D.check_view(D.view_records(1.0, np.radians(40.0), 0.0, H, W), H, W)
    # the training mode, module by module, is put back
    model.train()
    model.visual_encoder[1].eval()
    try:
        E.replay(model, ds, [3], 2)
        assert model.training and not model.visual_encoder[1].training
        assert model.visual_encoder[4].training
        with pytest.raises(RuntimeError):
            E.replay(model, ds, [N], 2)
        assert model.training and not model.visual_encoder[1].training
    finally:
        model.eval()
    rep = E.replay(model, ds, [3], 2)
    assert not model.training and not any(m.training for m in model.modules())
    # the JSON twin
    path = tmp_path / "replay.json"
    got = E.write_replay(str(path), model, ds, [3], 2, trace=True)
    doc = json.loads(path.read_text())
    assert doc["segments"] == json.loads(json.dumps(rep["segments"])) == \
        json.loads(json.dumps(got["segments"]))
    assert np.array(doc["trace"]["controls"]).shape == (2, 1, 3) and "view" not in doc["trace"]
