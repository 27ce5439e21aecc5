"""Evaluation harness: the metrics of the reference's evaluation_report.json (1-73), accumulated on
the device.

The reference publishes the report (overall MAE / MSE / RMSE / correlation per output, per-command
errors, steer |error| percentiles and accuracy buckets) but not the code that produced it; this
module emits the same JSON schema.  Every batch costs one eval forward (the HIP plan) plus one
`cilrs_eval_accumulate` launch that adds the batch's sums to a 72-double table in HBM; nothing is
copied to the host until `report()`.

`weather_sweep` and `view_sweep` score a checkpoint frame by frame under synthetic weather and from
displaced viewpoints, `adversarial_sweep` under the worst perturbation of a few 8-bit levels next to
a random one of the same size (csrc/adversarial.hip); `replay` closes the loop: recorded drives driven by the network's own steer,
with the state, the view records and the metrics on the device (csrc/replay.hip).
"""
from __future__ import annotations

import json

import numpy as np
import torch

from . import _lib as L

CHANNELS = ("Steer", "Throttle", "Brake", "Speed")
COMMANDS = ("FOLLOW", "LEFT", "RIGHT", "STRAIGHT")
PERCENTILES = (50, 75, 90, 95, 99)
BUCKETS = ("within_0.01", "within_0.02", "within_0.05", "within_0.1")


def _corr(n, sp, st, spt, spp, stt):
    cov = n * spt - sp * st
    vp = n * spp - sp * sp
    vt = n * stt - st * st
    return float(cov / np.sqrt(vp * vt)) if vp > 0 and vt > 0 else float("nan")


class Evaluator:
    """acc = Evaluator(model); acc.update(imgs, speeds, cmds, target_controls[, target_speed]);
    acc.report()"""

    def __init__(self, model, capacity: int = 1 << 16):
        self.model = model
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("Evaluator needs the model on an MI355X (no CPU fallback)")
        self.nacc = L.lib().cilrs_eval_acc_doubles()
        self.acc = torch.zeros(self.nacc, dtype=torch.float64, device=self.device)
        self.err = torch.empty(capacity, dtype=torch.float32, device=self.device)
        self.count = 0

    def reset(self):
        self.acc.zero_()
        self.count = 0

    def update_predictions(self, controls, pred_speed, target_controls, target_speed, command):
        """Accumulate already-computed predictions (device tensors)."""
        b = int(controls.size(0))
        if b == 0:
            return
        for t, shape in ((controls, (b, 3)), (target_controls, (b, 3)), (pred_speed, (b,)),
                         (target_speed, (b,)), (command, (b,))):
            if tuple(t.shape) != shape or t.device != self.device:
                raise RuntimeError(f"evaluate: expected shape {shape} on {self.device}, got "
                                   f"{tuple(t.shape)} on {t.device}")
        if command.dtype != torch.int64:
            raise RuntimeError("evaluate: command must be int64")
        if self.count + b > self.err.numel():                 # grow the |steer error| log
            grown = torch.empty(max(2 * self.err.numel(), self.count + b), dtype=torch.float32,
                                device=self.device)
            grown[:self.count] = self.err[:self.count]
            self.err = grown
        f32 = lambda t: t.to(torch.float32).contiguous()
        pc, ps, tc, ts = f32(controls), f32(pred_speed), f32(target_controls), f32(target_speed)
        cmd = command.contiguous()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_eval_accumulate(
            L.ptr(pc), L.ptr(ps), L.ptr(tc), L.ptr(ts), L.ptr(cmd), b, L.ptr(self.acc),
            L.C.c_void_p(self.err.data_ptr() + 4 * self.count), L.C.c_void_p(stream)))
        self.count += b

    def update(self, images, speeds, commands, target_controls, target_speed=None):
        """One validation batch: eval-mode forward, then accumulate.  target_speed defaults to the
        input speed (the reference trains the speed head to reproduce it,
        notebook/notebook.ipynb:550, 574)."""
        was_training = self.model.training
        self.model.eval()
        with torch.no_grad():
            pc, ps = self.model(images, speeds, commands)
        if was_training:
            self.model.train()
        self.update_predictions(pc, ps, target_controls,
                                speeds if target_speed is None else target_speed, commands)

    def report(self, checkpoint_epoch=None, model_name="CILRS (ResNet-34)"):
        """The evaluation_report.json dictionary (one device->host copy of the table and of the
        |steer error| log)."""
        a = self.acc.cpu().numpy()
        n_total = int(round(a[0]))
        overall = {}
        for c, name in enumerate(CHANNELS):
            n, sp, st, spt, spp, stt, sad, sdd = a[8 * c:8 * c + 8]
            if n == 0:
                raise RuntimeError("evaluate: no samples accumulated")
            mse = float(sdd / n)
            overall[name] = {"MAE": float(sad / n), "MSE": mse, "RMSE": float(np.sqrt(mse)),
                             "Correlation": _corr(n, sp, st, spt, spp, stt)}
        per_cmd = {}
        for k, cname in enumerate(COMMANDS):
            n, s0, s1, s2, sp, st, spt, spp, stt = a[32 + 9 * k:32 + 9 * k + 9]
            if n == 0:
                continue
            per_cmd[cname] = {"n": int(round(n)), "steer_mae": float(s0 / n),
                              "throttle_mae": float(s1 / n), "brake_mae": float(s2 / n),
                              "steer_corr": _corr(n, sp, st, spt, spp, stt)}
        err = self.err[:self.count].cpu().numpy().astype(np.float64)
        return {
            "model": model_name,
            "checkpoint_epoch": checkpoint_epoch,
            "val_samples": n_total,
            "overall_metrics": overall,
            "per_command_metrics": per_cmd,
            "steer_percentiles": {f"P{q}": float(np.percentile(err, q)) for q in PERCENTILES},
            "steer_accuracy_buckets": {b: float(a[68 + i] / n_total)
                                       for i, b in enumerate(BUCKETS)},
        }

    def write_json(self, path, **kw):
        rep = self.report(**kw)
        with open(path, "w") as f:
            json.dump(rep, f, indent=2)
        return rep


def evaluate(model, batches, **report_kw):
    """batches yields (images, speeds, commands, target_controls) like the reference's val_loader
    (notebook/notebook.ipynb:563-585)."""
    ev = Evaluator(model)
    for imgs, speeds, cmds, tgts in batches:
        ev.update(imgs, speeds, cmds, tgts)
    return ev.report(**report_kw)


def weather_sweep(model, dataset, indices, conditions=None, severities=(0.25, 0.5, 0.75, 1.0),
                  batch_size: int = 128, seed: int = 0, **report_kw):
    """How far the metrics move under synthetic weather, without a simulator: `evaluate` over
    `CachedBatchLoader(dataset, indices, train=False, weather=WeatherMix.fixed(name, severity))`
    for every (condition, severity) cell, and once with no weather.  dataset: a filled
    `DeviceDataset`.  conditions default to every name of `data.WEATHER_CONDITIONS` but "clear".

    -> {"clear": report, name: {severity: report}, "steer_mae": {"clear": mae, name: {severity:
    {"mae": mae, "ratio_to_clear": mae / clear mae}}}}.  The weather model is an image-space
    restatement (include/cilrs_hip.h), not CARLA's renderer."""
    from . import data as D
    conditions = D.WEATHER_CONDITIONS[1:] if conditions is None else tuple(conditions)
    for name in conditions:
        if name not in D.WEATHER_CONDITIONS:
            raise ValueError(f"unknown weather condition {name!r}; one of {D.WEATHER_CONDITIONS}")

    def run(mix):
        return evaluate(model, D.CachedBatchLoader(dataset, indices, batch_size, train=False,
                                                   seed=seed, weather=mix), **report_kw)

    def mae(rep):
        return rep["overall_metrics"]["Steer"]["MAE"]

    out = {"clear": run(None)}
    base = mae(out["clear"])
    table = {"clear": base}
    for name in conditions:
        out[name], table[name] = {}, {}
        for s in severities:
            s = float(s)
            rep = run(D.WeatherMix.fixed(name, s))
            out[name][s] = rep
            table[name][s] = {"mae": mae(rep),
                              "ratio_to_clear": mae(rep) / base if base > 0 else float("nan")}
    out["steer_mae"] = table
    return out


def _slope(xs, ys):
    """least-squares slope of ys over xs, or None with fewer than two distinct xs"""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    if len(xs) < 2 or np.ptp(xs) == 0:
        return None
    return float(np.polyfit(xs, ys, 1)[0])


def view_sweep(model, dataset, indices, lateral_m=(-1.0, -0.5, 0.0, 0.5, 1.0),
               yaw_deg=(-6.0, -3.0, 0.0, 3.0, 6.0), weather=None, batch_size: int = 128,
               seed: int = 0, **view_kw):
    """Does the checkpoint steer back when displaced -- without a simulator: one pass over
    `CachedBatchLoader(dataset, indices, train=False, weather=weather,
    view=ViewShift.fixed(lateral, yaw, **view_kw))` for every (lateral, yaw) cell, and one with no
    view (the centre).  dataset: a filled `DeviceDataset`; weather: a `WeatherMix` or None.

    -> {"centre": report, "cells": {lateral: {yaw: cell}}, "slopes": {...}} where a cell holds
      "report"       the evaluation report against the CORRECTED labels
      "steer_mae"    its steer MAE
      "steer_shift"  mean predicted steer minus the centre's
      "steer_delta"  mean correction the pure-pursuit rule asks for (`data.steer_correction`)
      "gain"         steer_shift / steer_delta, the response gain (None where the rule asks 0)
    and the slopes are least-squares fits of steer_shift: "steer_per_m" over the cells at yaw 0,
    "steer_per_deg" over the cells at lateral 0 (None when that row or column is not in the grid).
    A network that has only seen the lane centre is expected to show a gain near zero.  The warp
    is a flat-road model (include/cilrs_hip.h), not a renderer."""
    from . import data as D
    speeds = np.asarray(dataset.speed_host, dtype=np.float64)[np.asarray(indices)]
    steer_kw = {k: v for k, v in view_kw.items() if k != "camera"}

    def run(view):
        ev = Evaluator(model)
        for imgs, spd, cmds, tgts in D.CachedBatchLoader(dataset, indices, batch_size,
                                                         train=False, seed=seed, weather=weather,
                                                         view=view):
            ev.update(imgs, spd, cmds, tgts)
        a = ev.acc.cpu().numpy()
        return ev.report(), float(a[1] / a[0])               # steer: [n, Sp, ...]

    centre, centre_steer = run(None)
    out = {"centre": centre, "cells": {}}
    for lat in lateral_m:
        lat = float(lat)
        out["cells"][lat] = {}
        for yaw in yaw_deg:
            yaw = float(yaw)
            rep, steer = run(D.ViewShift.fixed(lat, yaw, **view_kw))
            delta = float(D.steer_correction(lat, np.radians(yaw), speeds, **steer_kw)
                          .astype(np.float32).mean(dtype=np.float64))
            shift = steer - centre_steer
            out["cells"][lat][yaw] = {
                "report": rep, "steer_mae": rep["overall_metrics"]["Steer"]["MAE"],
                "steer_shift": shift, "steer_delta": delta,
                "gain": shift / delta if delta != 0.0 else None}
    cells = out["cells"]
    lats, yaws = [float(v) for v in lateral_m], [float(v) for v in yaw_deg]
    out["slopes"] = {
        "steer_per_m": _slope(lats, [cells[v][0.0]["steer_shift"] for v in lats])
        if 0.0 in yaws else None,
        "steer_per_deg": _slope(yaws, [cells[0.0][v]["steer_shift"] for v in yaws])
        if 0.0 in lats else None}
    return out


def adversarial_sweep(model, dataset, indices, eps=(0.5, 1, 2, 4, 8), steps: int = 10,
                      output="steer", goal: str = "error", batch: int = 128, seed: int = 0,
                      **report_kw):
    """How far the metrics move under the WORST perturbation of at most eps 8-bit levels per byte
    (`adversarial.Attack`: PGD with `steps` steps, FGSM for steps = 1), next to a random-sign
    control of the same size -- without the control the figures cannot tell a worst-case
    perturbation from noise.  dataset: a filled `DeviceDataset`; goal "error" attacks w . (outputs -
    labels), "deviate" w . (outputs - clean prediction); `output` picks w as in
    `Predictor.saliency`.  The frames are scored as bytes: rounded, clipped, and through the same
    eval-mode forward as `evaluate`, so the eps = 0 row is the plain evaluation of those frames.

    -> {"clean": report, "eps": {eps: {"attack": row, "control": row}}, "steps", "goal", "seed"};
    a row holds "report" (the evaluation report on the perturbed bytes), "steer_mae",
    "dev_mean" / "dev_max" (|w . (outputs - reference)| over the frames), "share_over_0.1" (frames
    with |dev| > 0.1) and "linf_max" / "linf_mean" (levels actually moved)."""
    from .adversarial import Attack, attack_args
    from .predict import Predictor
    wts = Predictor._saliency_weights(output)
    if goal not in ("error", "deviate"):
        raise ValueError(f"adversarial_sweep: goal must be 'error' or 'deviate', got {goal!r}")
    cells = [attack_args(e, steps, None, None, goal, seed, "adversarial_sweep") for e in eps]
    if not dataset.filled:
        raise RuntimeError("adversarial_sweep: the dataset's cache is not filled (call fill())")
    index = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
    dataset.check_index(index)
    if index.size < 1 or batch < 1:
        raise ValueError("adversarial_sweep: no frames")
    eng = model.engine()
    if eng.train_precision != "fp32":
        raise RuntimeError("adversarial_sweep: fp32 plans only")
    dev = eng.device
    was_training = model.training
    model.eval()
    idx_dev = torch.from_numpy(index).to(dev)
    w_dev = torch.tensor(wts, dtype=torch.float64, device=dev)
    attacks = {}

    def batches():
        for b0 in range(0, index.size, batch):
            ids = idx_dev[b0:b0 + batch]
            yield (dataset.cache[ids], dataset.speed[ids], dataset.command_dev[ids],
                   dataset.targets[ids])

    def run(perturb):
        """One pass: perturb(attack, frames, spd, cmd, tgt) leaves bytes in attack.adv_u8."""
        ev = Evaluator(model)
        devs, linfs = [], []
        for frames, spd, cmd, tgt in batches():
            b = frames.size(0)
            if b not in attacks:
                attacks[b] = (Attack(eng, b, dataset.h, dataset.w),
                              torch.tensor(wts[:3], device=dev).expand(b, 3).contiguous(),
                              torch.full((b,), float(wts[3]), device=dev))
            at, dc, ds = attacks[b]
            ref = perturb(at, frames, spd, cmd, tgt, dc, ds)
            with torch.no_grad():
                pc, ps = model(at.clean_input(at.adv_u8, out=at.g), spd, cmd)
            ev.update_predictions(pc, ps, tgt, spd, cmd)
            d = torch.cat([pc - ref[0], (ps - ref[1])[:, None]], 1).double() @ w_dev
            devs.append(d.abs())
            linfs.append(at.linf.clone())
        d = torch.cat(devs).cpu().numpy()
        li = torch.cat(linfs).cpu().numpy()
        rep = ev.report(**report_kw)
        return {"report": rep, "steer_mae": rep["overall_metrics"]["Steer"]["MAE"],
                "dev_mean": float(d.mean()), "dev_max": float(d.max()),
                "share_over_0.1": float((d > 0.1).mean()), "linf_max": int(li.max()),
                "linf_mean": float(li.mean())}

    def reference(at, tgt, spd):
        if goal == "error":
            return tgt, spd
        return at.ctrl0.clone(), at.spd0.clone()

    out = {"eps": {}, "steps": int(steps), "goal": goal, "seed": int(seed)}
    try:
        for e, n, alpha, rs, _, sd in cells:
            def attack(at, frames, spd, cmd, tgt, dc, ds):
                at.run(frames, spd, cmd, dc, ds, wts, e, n, alpha, rs, goal, sd,
                       targets=(tgt, spd) if goal == "error" else None, score=False)
                return reference(at, tgt, spd)

            def control(at, frames, spd, cmd, tgt, dc, ds):
                if goal != "error":
                    eng.run_forward_frozen_u8(frames, spd, cmd, out=(at.ctrl0, at.spd0))
                at.random_sign_control(frames, e, sd)
                return reference(at, tgt, spd)
            out["eps"][e] = {"attack": run(attack), "control": run(control)}
        out["clean"] = evaluate(model, _clean_batches(eng, batches), **report_kw)
    finally:
        if was_training:
            model.train()
    return out


def _clean_batches(eng, batches):
    """The frames of a sweep as `evaluate` takes them: preprocessed, no perturbation."""
    for frames, spd, cmd, tgt in batches():
        yield eng.run_attr_samples(frames, None, 0, 1, 0, 1, 0.0, 0), spd, cmd, tgt


# ---- closed-loop replay -------------------------------------------------------------------------
# the metrics row of `cilrs_replay_step` (include/cilrs_hip.h), in its order
REPLAY_METRICS = ("ticks", "lateral_interventions", "yaw_interventions", "nonfinite", "sum_abs_e",
                  "sum_e2", "max_abs_e", "sum_abs_psi", "max_abs_psi", "sum_abs_steer_err",
                  "sum_abs_steer_err_corrected", "sum_dsteer2", "recover_tick", "steer_ticks")
REPLAY_MAX_TAPS = 8
REPLAY_FLAGS = {"lateral": 1, "yaw": 2, "nonfinite": 4, "view_on": 8}


def _replay_summary(m: dict, dt: float, penalty_s: float) -> dict:
    """per-segment (or summed) metrics -> the derived figures"""
    ticks, steer = m["ticks"], m["steer_ticks"]
    n_int = m["lateral_interventions"] + m["yaw_interventions"] + m["nonfinite"]
    out = dict(m)
    out["interventions"] = n_int
    out["autonomy"] = max(0.0, 1.0 - penalty_s * n_int / (ticks * dt)) if ticks > 0 else None
    out["mean_abs_e"] = m["sum_abs_e"] / ticks if ticks > 0 else None
    out["rms_e"] = float(np.sqrt(m["sum_e2"] / ticks)) if ticks > 0 else None
    out["mean_abs_psi"] = m["sum_abs_psi"] / ticks if ticks > 0 else None
    out["steer_mae"] = m["sum_abs_steer_err"] / steer if steer > 0 else None
    out["steer_mae_corrected"] = m["sum_abs_steer_err_corrected"] / steer if steer > 0 else None
    return out


def replay(model, dataset, starts, ticks, *, lateral_m=0.0, yaw_deg=0.0, dt=0.05,
           max_lateral_m=1.0, max_yaw_deg=10.0, recover_m=0.1, penalty_s=6.0, steer_filter=(),
           closed_loop=True, weather=None, seed=0, camera=None, trace=False, batch_size=128,
           **steer_kw):
    """Closed-loop replay of recorded drives, without a simulator (PilotNet's re-simulator on the
    device; the definition is in include/cilrs_hip.h, "closed-loop replay").  Every segment
    `starts[s] .. starts[s] + ticks` of `dataset` (a filled `DeviceDataset`; consecutive frames of
    one drive, see `data.drive_ranges`) is driven by the model's steer: a kinematic bicycle moves the
    car off the recorded path by (e metres, psi radians), the next recorded frame is shown from
    there (`cilrs_batch_assemble_view`; speed and command stay the recorded ones), and leaving the
    box (+-max_lateral_m, +-max_yaw_deg) is an intervention that puts the car back on the path.
    Segments start at (`lateral_m`, `yaw_deg`), scalars or one value per segment.

    A tick is three launches on the current stream -- `cilrs_replay_step`, the assemble, the eval
    forward -- and no host synchronisation; `batch_size` segments run at once; the results are read
    back once at the end.  steer_filter: 0 to 8 weights, oldest to newest, of a running weighted
    mean of the predicted steer (the reference agent's `smooth_steering`,
    model/autonomous_drive.py:925-932, is (0.1, 0.15, 0.2, 0.25, 0.3)).  closed_loop=False keeps
    every segment at its start pose: a `view_sweep` cell over consecutive frames.  weather: a
    `WeatherMix`, its [ticks, segments] records drawn up front from `seed`.  steer_kw: the
    arguments of `data.steer_correction` (the vehicle and the look-ahead).

    Limits of the model: the small-offset Frenet form (the factor cos(psi) / (1 - e kappa) on the
    expert's curvature is dropped); longitudinal motion stays the expert's (throttle and brake are
    not simulated); the warp is a flat-road model.

    -> {"config", "segments": [per-segment metrics, "autonomy" = max(0, 1 - penalty_s *
    interventions / (ticks * dt)), ...], "overall"}; with trace=True also "trace": per tick
    [ticks, segments] "e", "psi", "raw_steer", "steer", "flags" (`REPLAY_FLAGS`), "controls"
    [ticks, segments, 3], "index" and the raw view records "view" (VIEW_DTYPE)."""
    from . import data as D
    ticks = int(ticks)
    if ticks < 1:
        raise RuntimeError("replay: ticks must be at least 1")
    if not getattr(dataset, "filled", False):
        raise RuntimeError("replay: the dataset's cache is not filled (call fill())")
    if getattr(dataset, "speed_host", None) is None \
            or not np.isfinite(np.asarray(dataset.speed_host, dtype=np.float64)).all():
        raise RuntimeError("replay: needs the dataset's host speeds (speed_host), all finite")
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.int64).reshape(-1))
    n_seg, n, h, w = len(starts), len(dataset), dataset.h, dataset.w
    if n_seg < 1:
        raise RuntimeError("replay: no segments")
    if int(starts.min()) < 0 or int(starts.max()) + ticks > n:
        bad = starts[(starts < 0) | (starts + ticks > n)][0]
        raise RuntimeError(f"replay: segment [{int(bad)}, {int(bad) + ticks}) outside the "
                           f"dataset's [0, {n})")
    taps = [float(t) for t in steer_filter]
    if len(taps) > REPLAY_MAX_TAPS:
        raise RuntimeError(f"replay: {len(taps)} filter taps, at most {REPLAY_MAX_TAPS}")
    if taps and (not np.isfinite(taps).all() or min(taps) < 0 or not taps[-1] > 0):
        raise RuntimeError("replay: filter taps must be finite and non-negative, the newest positive")
    if batch_size < 1:
        raise RuntimeError("replay: batch_size must be at least 1")
    lat0 = np.ascontiguousarray(np.broadcast_to(np.asarray(lateral_m, dtype=np.float64), (n_seg,)))
    yaw0 = np.ascontiguousarray(np.radians(np.broadcast_to(
        np.asarray(yaw_deg, dtype=np.float64), (n_seg,))))
    camera = D.CameraModel() if camera is None else camera
    D.steer_correction(0.0, 0.0, 0.0, **steer_kw)              # refuses an unknown argument now
    max_yaw_rad = float(np.radians(max_yaw_deg))
    if not (max_lateral_m > 0 and 0 < max_yaw_rad < 1.5 and dt > 0 and recover_m >= 0):
        raise RuntimeError("replay: max_lateral_m, max_yaw_deg (below 85) and dt must be positive, "
                           "recover_m non-negative")
    if not (np.isfinite(lat0).all() and np.isfinite(yaw0).all()
            and (np.abs(lat0) <= max_lateral_m).all() and (np.abs(yaw0) <= max_yaw_rad).all()):
        raise RuntimeError("replay: a segment starts outside the box (+-max_lateral_m, "
                           "+-max_yaw_deg)")
    # every record the loop can write lies in the box: w of both matrices depends on psi only and
    # |steer_delta| falls with the look-ahead, so the four corners at standstill bound them all
    D.check_view(D.view_records([max_lateral_m, max_lateral_m, -max_lateral_m, -max_lateral_m],
                                [max_yaw_rad, -max_yaw_rad, max_yaw_rad, -max_yaw_rad], 0.0, h, w,
                                camera, **steer_kw), h, w)
    if weather is not None and w > D.WEATHER_MAX_WIDTH:
        raise RuntimeError(f"weather: width {w} above {D.WEATHER_MAX_WIDTH}")
    dev = dataset.device
    if next(model.parameters()).device != dev:
        raise RuntimeError("replay: model and dataset must be on the same GPU (no CPU fallback)")

    kw = dict(lookahead_s=1.0, min_lookahead_m=4.0, wheelbase_m=2.875, max_steer_deg=70.0)
    kw.update(steer_kw)
    fx, fy, cx, cy = camera.intrinsics(h, w)
    cfg = L.ReplayConfig(
        dt_s=float(dt), speed_unit_ms=D.SPEED_NORM_KMH / 3.6, wheelbase_m=float(kw["wheelbase_m"]),
        max_wheel_rad=float(np.radians(kw["max_steer_deg"])), lookahead_s=float(kw["lookahead_s"]),
        min_lookahead_m=float(kw["min_lookahead_m"]), fx=fx, fy=fy, cx=cx, cy=cy,
        height_m=camera.height_m, max_lateral_m=float(max_lateral_m), max_yaw_rad=max_yaw_rad,
        recover_m=float(recover_m), taps=(L.C.c_double * 8)(*taps), ntaps=len(taps),
        closed_loop=1 if closed_loop else 0)
    lib = L.lib()
    ns, nm = lib.cilrs_replay_state_doubles(), lib.cilrs_replay_metric_doubles()
    assert nm == len(REPLAY_METRICS)
    vsz, wsz = D.VIEW_DTYPE.itemsize, D.WEATHER_DTYPE.itemsize
    wrng = np.random.default_rng([seed, D.WEATHER_STREAM])
    vp = L.C.c_void_p
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    kept = []
    try:
        with torch.no_grad():
            for b0 in range(0, n_seg, batch_size):
                b = min(batch_size, n_seg - b0)
                stream = vp(torch.cuda.current_stream(dev).cuda_stream)
                state = torch.empty(b, ns, dtype=torch.float64, device=dev)
                metrics = torch.empty(b, nm, dtype=torch.float64, device=dev)
                index = torch.empty(ticks, b, dtype=torch.int64, device=dev)
                view = torch.empty(ticks, b, vsz, dtype=torch.uint8, device=dev)
                pdev = D._records_to_device(D.identity_params(b), dev)
                wdev = None
                if weather is not None:
                    wrec = weather.draw(wrng, ticks * b, h, w)
                    D.check_weather(wrec, h, w)
                    wdev = D._records_to_device(wrec, dev).view(ticks, b, wsz)
                tr = None
                if trace:
                    tr = (torch.empty(ticks, b, 2, dtype=torch.float64, device=dev),
                          torch.empty(ticks, b, 2, dtype=torch.float32, device=dev),
                          torch.empty(ticks, b, dtype=torch.uint8, device=dev), [])

                def row(k):                  # the trace rows of tick k
                    return (None,) * 3 if tr is None else tuple(L.ptr(t[k]) for t in tr[:3])
                L.check(lib.cilrs_replay_begin(
                    L.C.byref(cfg), b, ticks, n, vp(starts[b0:b0 + b].ctypes.data),
                    vp(lat0[b0:b0 + b].ctypes.data), vp(yaw0[b0:b0 + b].ctypes.data),
                    L.ptr(dataset.speed), L.ptr(state), L.ptr(metrics), L.ptr(index[0]),
                    L.ptr(view[0]), stream))
                controls = None
                for k in range(ticks):
                    if k >= 1:
                        L.check(lib.cilrs_replay_step(
                            L.C.byref(cfg), b, k, L.ptr(controls), L.ptr(dataset.speed),
                            L.ptr(dataset.targets), n, L.ptr(state), L.ptr(metrics),
                            L.ptr(index[k]), L.ptr(view[k]), *row(k - 1), stream))
                    img, spd, cmd, _tgt = dataset._launch(
                        index[k].data_ptr(), pdev.data_ptr(), b,
                        weather_ptr=None if wdev is None else wdev[k].data_ptr(),
                        view_ptr=view[k].data_ptr())
                    controls, _speed = model(img, spd, cmd)
                    if controls.dtype != torch.float32 or tuple(controls.shape) != (b, 3) \
                            or not controls.is_contiguous() or controls.device != dev:
                        raise RuntimeError("replay: the model must return contiguous float32 "
                                           "[B, 3] controls on the dataset's GPU")
                    if tr is not None:
                        tr[3].append(controls)
                L.check(lib.cilrs_replay_finish(
                    L.C.byref(cfg), b, ticks, L.ptr(controls), L.ptr(dataset.speed),
                    L.ptr(dataset.targets), n, L.ptr(state), L.ptr(metrics), *row(ticks - 1),
                    stream))
                kept.append((metrics, index, view, tr))
    finally:
        for m, t in modes:
            m.training = t
        if modes[0][1] and hasattr(model, "weights_changed"):
            model.weights_changed()
    # the one read-back
    table = torch.cat([k[0] for k in kept]).cpu().numpy()
    segments = []
    for s in range(n_seg):
        m = {name: float(table[s, j]) for j, name in enumerate(REPLAY_METRICS)}
        for name in ("ticks", "lateral_interventions", "yaw_interventions", "nonfinite",
                     "recover_tick", "steer_ticks"):
            m[name] = int(m[name])
        seg = _replay_summary(m, float(dt), float(penalty_s))
        seg.update(start=int(starts[s]), lateral0_m=float(lat0[s]), yaw0_rad=float(yaw0[s]))
        segments.append(seg)
    total = {name: (max if name.startswith("max_") else sum)(g[name] for g in segments)
             for name in REPLAY_METRICS if name != "recover_tick"}
    overall = _replay_summary(total, float(dt), float(penalty_s))
    rec = [g["recover_tick"] for g in segments if abs(g["lateral0_m"]) >= recover_m]
    overall["segments"] = n_seg
    overall["started_outside"] = len(rec)
    overall["recovered"] = sum(r >= 0 for r in rec)
    overall["mean_recover_tick"] = float(np.mean([r for r in rec if r >= 0])) \
        if any(r >= 0 for r in rec) else None
    out = {"config": {"ticks": ticks, "dt": float(dt), "max_lateral_m": float(max_lateral_m),
                      "max_yaw_deg": float(max_yaw_deg), "recover_m": float(recover_m),
                      "penalty_s": float(penalty_s), "steer_filter": taps,
                      "closed_loop": bool(closed_loop), "seed": int(seed),
                      "weather": None if weather is None else
                      {"names": list(weather.names), "severity": list(weather.severity)},
                      "camera": {"width0": camera.width0, "height0": camera.height0,
                                 "fov_deg": camera.fov_deg, "height_m": camera.height_m},
                      "steer": {k: float(v) for k, v in kw.items()}},
           "segments": segments, "overall": overall}
    if trace:
        cat = lambda ts: torch.cat(ts, dim=1).cpu().numpy()
        st = cat([k[3][0] for k in kept])
        steer = cat([k[3][1] for k in kept])
        out["trace"] = {
            "e": st[..., 0], "psi": st[..., 1], "raw_steer": steer[..., 0], "steer": steer[..., 1],
            "flags": cat([k[3][2] for k in kept]),
            "controls": cat([torch.stack(k[3][3]) for k in kept]),
            "index": cat([k[1] for k in kept]),
            "view": np.ascontiguousarray(cat([k[2] for k in kept])).view(D.VIEW_DTYPE)[..., 0]}
    return out


def write_replay(path, model, dataset, starts, ticks, **kw):
    """`replay` written as JSON (a trace's arrays become lists; its raw view records are left
    out)."""
    rep = replay(model, dataset, starts, ticks, **kw)
    doc = dict(rep)
    if "trace" in doc:
        doc["trace"] = {k: v.tolist() for k, v in doc["trace"].items() if k != "view"}
    with open(path, "w") as f:
        json.dump(doc, f, indent=2)
    return rep


def write_view_sweep(path, model, dataset, indices, **kw):
    """`view_sweep` written as JSON (offsets and yaws become string keys)."""
    rep = view_sweep(model, dataset, indices, **kw)
    with open(path, "w") as f:
        json.dump(rep, f, indent=2)
    return rep


def write_weather_sweep(path, model, dataset, indices, **kw):
    """`weather_sweep` written as JSON (severities become string keys)."""
    rep = weather_sweep(model, dataset, indices, **kw)
    with open(path, "w") as f:
        json.dump(rep, f, indent=2)
    return rep


def write_adversarial_sweep(path, model, dataset, indices, **kw):
    """`adversarial_sweep` written as JSON (the eps values become string keys)."""
    rep = adversarial_sweep(model, dataset, indices, **kw)
    with open(path, "w") as f:
        json.dump(rep, f, indent=2)
    return rep
