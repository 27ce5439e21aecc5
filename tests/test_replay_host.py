"""Closed-loop replay on the host: the float64 definition (tests/_replay.py) under a pure-pursuit
controller that must recover and one that must not, the edges of the definition (the limit itself,
the filter, the clip, a stopped car), the C-ABI's layout, and `data.drive_ranges`."""
import ctypes
import math
import os

import numpy as np
import pytest

import _replay as RP
from test_host import make_sessions

T = 400
SPEEDS = (0.1, 0.25, 0.5, 1.0)
STARTS = ((0.5, 0.0), (-0.5, 3.0), (0.9, -5.0), (0.0, 8.0))
RISING = (1.0, 2.0, 3.0, 4.0, 5.0)


def _drive(v_n, taps=(), **kw):
    speed = np.full(T, v_n, dtype=np.float32)
    targets = np.zeros((T, 3), dtype=np.float32)
    targets[:, 0] = 0.05 * np.sin(np.arange(T) / 30.0)
    return RP.Config(steer_filter=taps, **kw), speed, targets


def _pursuit(sign):
    from cilrs_mi355 import data as D
    return lambda k, e, psi, v_n, sx: sx + sign * float(D.steer_correction(e, psi, v_n))


def test_layout_matches_the_library():
    from cilrs_mi355 import _lib as L
    from cilrs_mi355 import evaluate as E
    assert ctypes.sizeof(L.ReplayConfig) == 184
    assert E.REPLAY_METRICS == RP.METRICS
    assert E.REPLAY_FLAGS == {"lateral": RP.FLAG_LATERAL, "yaw": RP.FLAG_YAW,
                              "nonfinite": RP.FLAG_NONFINITE, "view_on": RP.FLAG_ON}
    lib = ctypes.CDLL(L.LIB_PATH)
    assert lib.cilrs_replay_metric_doubles() == len(RP.METRICS)
    assert lib.cilrs_replay_state_doubles() >= 2 + 1 + E.REPLAY_MAX_TAPS


@pytest.mark.parametrize("taps", [(), RISING], ids=["no filter", "rising 5 taps"])
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("v_n", SPEEDS)
def test_pure_pursuit_recovers(v_n, start, taps):
    cfg, speed, targets = _drive(v_n, taps)
    seg, rows = RP.replay(cfg, 0, start[0], math.radians(start[1]), speed, targets, _pursuit(+1), T)
    m = seg.m
    assert m["ticks"] == T == m["steer_ticks"]
    assert m["lateral_interventions"] == m["yaw_interventions"] == m["nonfinite"] == 0
    e = np.abs([r[0] for r in rows])
    outside = np.nonzero(e >= 0.1)[0]
    settled = 0 if len(outside) == 0 else int(outside[-1]) + 1
    print(f"v_n {v_n} start {start} taps {len(taps)}: |e| < 0.1 from tick {settled}, "
          f"max |e| {e.max():.3f}")
    assert settled <= 150, settled
    if abs(start[0]) >= cfg.recover_m:
        assert 0 < m["recover_tick"] <= settled and e[int(m["recover_tick"])] < 0.1
        assert (e[:int(m["recover_tick"])] >= 0.1).all()
    else:
        assert m["recover_tick"] == -1
    assert m["max_abs_e"] == e.max() and m["sum_abs_e"] == pytest.approx(e.sum(), rel=1e-12)
    # the record of every displaced tick is on and carries the pose
    for r in rows:
        rec = r[5]
        assert rec["on"][0] == (0 if r[0] == 0.0 and r[1] == 0.0 else 1)
        assert rec["lateral_m"][0] == np.float32(r[0]) and rec["yaw_rad"][0] == np.float32(r[1])


@pytest.mark.parametrize("taps", [(), RISING], ids=["no filter", "rising 5 taps"])
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("v_n", SPEEDS)
def test_steering_away_is_intervened(v_n, start, taps):
    cfg, speed, targets = _drive(v_n, taps)
    seg = RP.Segment(cfg, start[0], math.radians(start[1]))
    steer = _pursuit(-1)
    hits = 0
    for k in range(T):
        raw = steer(k, seg.e, seg.psi, float(speed[k]), RP.clip1(float(targets[k, 0])))
        _s, flags = seg.advance(raw, speed[k], targets[k, 0])
        if flags & (RP.FLAG_LATERAL | RP.FLAG_YAW):
            hits += 1
            assert seg.e == 0.0 and seg.psi == 0.0 and seg.hist == [] and seg.prev is None
            assert not math.copysign(1.0, seg.e) < 0 and not math.copysign(1.0, seg.psi) < 0
    m = seg.m
    assert hits >= 1 and hits == m["lateral_interventions"] + m["yaw_interventions"]
    assert m["nonfinite"] == 0 and m["ticks"] == T
    assert m["max_abs_e"] <= cfg.max_lateral_m and m["max_abs_psi"] <= cfg.max_yaw_rad
    assert m["recover_tick"] == -1 or abs(start[0]) >= cfg.recover_m


def test_exactly_at_the_limit_is_no_intervention():
    cfg, speed, targets = _drive(0.5)
    seg = RP.Segment(cfg, cfg.max_lateral_m, 0.0)
    s, flags = seg.advance(float(targets[0, 0]), speed[0], targets[0, 0])     # steers as the expert
    assert flags == RP.FLAG_ON and seg.e == cfg.max_lateral_m and seg.psi == 0.0
    # a hair beyond it is one
    seg = RP.Segment(cfg, cfg.max_lateral_m, 1e-9)
    _s, flags = seg.advance(0.0, speed[0], 0.0)
    assert flags == RP.FLAG_ON | RP.FLAG_LATERAL and (seg.e, seg.psi) == (0.0, 0.0)
    # the yaw limit, from the inside and beyond
    seg = RP.Segment(cfg, 0.0, cfg.max_yaw_rad)
    _s, flags = seg.advance(0.0, 0.0, 0.0)                                   # standing: stays
    assert flags == RP.FLAG_ON and seg.psi == cfg.max_yaw_rad
    _s, flags = seg.advance(0.5, speed[0], 0.0)                              # turns further right
    assert flags == RP.FLAG_ON | RP.FLAG_YAW and (seg.e, seg.psi) == (0.0, 0.0)


def test_filter_with_one_to_ntaps_entries():
    taps = (0.5, 1.0, 2.0, 4.0)
    cfg, speed, targets = _drive(0.0, taps)
    seg = RP.Segment(cfg)
    raws = [0.3, -0.2, 0.1, 0.05, -0.4, 0.25]
    for k, raw in enumerate(raws):
        s, _f = seg.advance(raw, 0.0, 0.0)
        held = raws[max(0, k + 1 - len(taps)):k + 1]
        w = taps[len(taps) - len(held):]
        want = raw if len(held) == 1 else sum(a * b for a, b in zip(w, held)) / sum(w)
        assert seg.hist == held and s == pytest.approx(want, rel=1e-15, abs=0)
        if len(held) == 1:
            assert s == raw
    # a non-finite steer empties it; the next value stands alone again
    s, flags = seg.advance(math.nan, 0.0, 0.0)
    assert math.isnan(s) and flags == RP.FLAG_NONFINITE and seg.hist == []
    s, _f = seg.advance(0.7, 0.0, 0.0)
    assert s == 0.7 and seg.hist == [0.7]
    assert seg.m["nonfinite"] == 1 and seg.m["steer_ticks"] == len(raws) + 1
    # no taps: no history at all
    seg = RP.Segment(_drive(0.0)[0])
    assert seg.advance(0.3, 0.0, 0.0)[0] == 0.3 and seg.hist == []


def test_steer_is_clipped():
    cfg, speed, targets = _drive(0.5)
    for raw, want in ((3.0, 1.0), (-3.0, -1.0)):
        seg = RP.Segment(cfg, 0.0, 0.0)
        s, flags = seg.advance(raw, 0.05, 0.0)
        assert s == want and flags == 0
        ds = (0.05 * cfg.speed_unit_ms) * cfg.dt_s
        assert seg.e == 0.0 and seg.psi == want * ds * math.tan(cfg.max_wheel_rad) / cfg.wheelbase_m
        assert seg.m["sum_abs_steer_err"] == 1.0
    # the label is clipped too: beyond the lock on both sides, nothing turns
    seg = RP.Segment(cfg, 0.2, 0.0)
    seg.advance(3.0, 0.5, 2.5)
    assert (seg.e, seg.psi) == (0.2, 0.0)


def test_a_stopped_car_stays():
    cfg, speed, targets = _drive(0.0, RISING)
    seg = RP.Segment(cfg, 0.4, math.radians(-3.0))
    for k in range(20):
        seg.advance(0.9 * (-1) ** k, 0.0, 0.1)
    assert (seg.e, seg.psi) == (0.4, math.radians(-3.0))
    assert seg.m["ticks"] == 20 and seg.m["lateral_interventions"] + seg.m["yaw_interventions"] == 0
    assert seg.m["sum_abs_e"] == pytest.approx(20 * 0.4, rel=1e-14)


def test_open_loop_keeps_the_start_pose():
    cfg, speed, targets = _drive(1.0, closed_loop=False)
    seg, rows = RP.replay(cfg, 0, 0.3, math.radians(2.0), speed, targets, _pursuit(-1), 50)
    assert all(r[0] == 0.3 and r[1] == math.radians(2.0) for r in rows)
    assert seg.m["ticks"] == 50 and seg.m["lateral_interventions"] == 0
    assert seg.m["sum_abs_steer_err_corrected"] > seg.m["sum_abs_steer_err"] > 0


def test_drive_ranges_split_at_sessions_and_missing_frames(tmp_path):
    from cilrs_mi355 import data as D
    root = str(tmp_path)
    make_sessions(root, (7, 5))
    s = D.Sessions(root)
    assert D.drive_ranges(s) == [(0, 7), (7, 12)]
    # the recorder skipped frame 3 of session 1 and frames 1, 2 of session 2
    keep = np.array([i for i in range(12) if i not in (3, 8, 9)])
    s.paths = s.paths[keep]
    assert [os.path.basename(p) for p in s.paths[2:4]] == ["frame_00000002.jpg",
                                                           "frame_00000004.jpg"]
    assert D.drive_ranges(s) == [(0, 3), (3, 6), (6, 7), (7, 9)]
    assert D.drive_ranges(s, max_gap=2) == [(0, 6), (6, 7), (7, 9)]
    assert D.drive_ranges(s, max_gap=3) == [(0, 6), (6, 9)]
    with pytest.raises(ValueError):
        D.drive_ranges(s, max_gap=0)
