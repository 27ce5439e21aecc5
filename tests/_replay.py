"""The closed-loop replay of include/cilrs_hip.h ("closed-loop replay") in float64 numpy, one
segment at a time: what csrc/replay.hip is compared against (test_replay_gpu.py) and what the
controller tests drive on the host (test_replay_host.py).

Tick k on frame i = start + k:
  render   the record is `identity_view` where e == 0 and psi == 0, else what
           `view_records(e, psi, speed[i], H, W, camera, **steer_kw)` gives;
  advance  `Segment.advance(raw, v_n, label)`: the metrics of the tick, the steer filter, the clip,
           the bicycle step and the interventions, in the order the header gives them.
Sums run sequentially in Python floats (IEEE double, one rounding per operation), never through a
numpy reduction whose order is its own."""
import math

import numpy as np

STATE_E, STATE_PSI = 0, 1
METRICS = ("ticks", "lateral_interventions", "yaw_interventions", "nonfinite", "sum_abs_e",
           "sum_e2", "max_abs_e", "sum_abs_psi", "max_abs_psi", "sum_abs_steer_err",
           "sum_abs_steer_err_corrected", "sum_dsteer2", "recover_tick", "steer_ticks")
FLAG_LATERAL, FLAG_YAW, FLAG_NONFINITE, FLAG_ON = 1, 2, 4, 8


def clip1(v):
    return min(max(v, -1.0), 1.0)


class Config:
    def __init__(self, dt=0.05, max_lateral_m=1.0, max_yaw_deg=10.0, recover_m=0.1,
                 steer_filter=(), closed_loop=True, camera=None, height=88, width=200, **steer_kw):
        from cilrs_mi355 import data as D
        self.D = D
        self.dt_s = float(dt)
        self.speed_unit_ms = D.SPEED_NORM_KMH / 3.6
        kw = dict(lookahead_s=1.0, min_lookahead_m=4.0, wheelbase_m=2.875, max_steer_deg=70.0)
        kw.update(steer_kw)
        self.steer_kw = steer_kw
        self.wheelbase_m = float(kw["wheelbase_m"])
        self.max_wheel_rad = float(np.radians(kw["max_steer_deg"]))
        self.max_lateral_m = float(max_lateral_m)
        self.max_yaw_rad = float(np.radians(max_yaw_deg))
        self.recover_m = float(recover_m)
        self.taps = [float(w) for w in steer_filter]
        self.closed_loop = bool(closed_loop)
        self.camera = D.CameraModel() if camera is None else camera
        self.height, self.width = height, width

    def record(self, e, psi, v_n):
        """the view record of a tick rendered at (e, psi), VIEW_DTYPE [1]"""
        if e == 0.0 and psi == 0.0:
            return self.D.identity_view(1)
        return self.D.view_records(e, psi, v_n, self.height, self.width, self.camera,
                                   **self.steer_kw)

    def delta(self, e, psi, v_n):
        """the correction the pure-pursuit rule asks for, in double (0 on the path)"""
        if e == 0.0 and psi == 0.0:
            return 0.0
        return float(self.D.steer_correction(e, psi, v_n, **self.steer_kw))


class Segment:
    def __init__(self, cfg: Config, lateral0=0.0, yaw0=0.0):
        self.cfg = cfg
        self.e, self.psi = float(lateral0), float(yaw0)
        self.lateral0, self.yaw0 = self.e, self.psi
        self.hist = []
        self.prev = None
        self.recover_open = abs(self.e) >= cfg.recover_m
        self.m = dict.fromkeys(METRICS, 0.0)
        self.m["recover_tick"] = -1.0
        self.tick = 0

    def filtered(self, raw):
        """raw joins the history; the weighted mean over what the history holds"""
        c = self.cfg
        n_taps = len(c.taps)
        if n_taps > 0:
            self.hist = (self.hist + [raw])[-n_taps:]
        n = len(self.hist)
        if n_taps == 0 or n == 1:
            return raw
        num = den = 0.0
        for w, h in zip(c.taps[n_taps - n:], self.hist):
            num += w * h
            den += w
        return num / den

    def advance(self, raw, v_n, label):
        """one tick: controls[b][0], speed[i] and targets[i][0] as Python floats -> (applied steer
        or NaN, flags)"""
        c, m = self.cfg, self.m
        raw, v_n = float(raw), float(v_n)
        sx = clip1(float(label))
        e, psi = self.e, self.psi
        on = not (e == 0.0 and psi == 0.0)
        delta = c.delta(e, psi, v_n)
        m["ticks"] += 1.0
        m["sum_abs_e"] += abs(e)
        m["sum_e2"] += e * e
        m["max_abs_e"] = max(m["max_abs_e"], abs(e))
        m["sum_abs_psi"] += abs(psi)
        m["max_abs_psi"] = max(m["max_abs_psi"], abs(psi))
        if self.recover_open and abs(e) < c.recover_m:
            m["recover_tick"] = float(self.tick)
            self.recover_open = False
        flags = FLAG_ON if on else 0
        intervene = False
        s = math.nan
        if not math.isfinite(raw):
            m["nonfinite"] += 1.0
            flags |= FLAG_NONFINITE
            intervene = True
        else:
            s = clip1(self.filtered(raw))
            m["steer_ticks"] += 1.0
            m["sum_abs_steer_err"] += abs(s - sx)
            m["sum_abs_steer_err_corrected"] += abs(s - clip1(sx + delta))
            if self.prev is not None:
                d = s - self.prev
                m["sum_dsteer2"] += d * d
            self.prev = s
            if c.closed_loop:
                ds = (v_n * c.speed_unit_ms) * c.dt_s
                e2 = e + ds * math.sin(psi)
                p2 = psi + ds * (math.tan(s * c.max_wheel_rad)
                                 - math.tan(sx * c.max_wheel_rad)) / c.wheelbase_m
                if not (math.isfinite(e2) and math.isfinite(p2)):
                    m["nonfinite"] += 1.0
                    flags |= FLAG_NONFINITE
                    intervene = True
                elif abs(e2) > c.max_lateral_m:
                    m["lateral_interventions"] += 1.0
                    flags |= FLAG_LATERAL
                    intervene = True
                elif abs(p2) > c.max_yaw_rad:
                    m["yaw_interventions"] += 1.0
                    flags |= FLAG_YAW
                    intervene = True
                else:
                    self.e, self.psi = e2, p2
        if intervene:
            if c.closed_loop:
                self.e = self.psi = 0.0
            self.hist = []
            self.prev = None
            self.recover_open = False
        self.tick += 1
        return s, flags

    def metrics(self):
        return np.array([self.m[k] for k in METRICS], dtype=np.float64)


def replay(cfg: Config, start, lateral0, yaw0, speed, targets, controller, ticks):
    """One segment over `ticks` frames from `start`: controller(k, e, psi, v_n, sx) -> raw steer.
    -> (segment, rows) with a row (e, psi, raw, s, flags, record) per tick."""
    seg = Segment(cfg, lateral0, yaw0)
    rows = []
    for k in range(ticks):
        i = start + k
        v_n, label = float(speed[i]), float(targets[i][0])
        e, psi = seg.e, seg.psi
        rec = cfg.record(e, psi, v_n)
        raw = float(controller(k, e, psi, v_n, clip1(label)))
        s, flags = seg.advance(raw, v_n, label)
        rows.append((e, psi, raw, s, flags, rec))
    return seg, rows
