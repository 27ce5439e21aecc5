#!/usr/bin/env python3
"""What moving the closed-loop replay's state onto the device buys, on synthetic frames at 88x200.

Two loops over the same segments, T ticks each, B segments at once, a random-init CILRS in eval
mode (fp32), no steer filter, no weather:

  device  `evaluate.replay`: per tick `cilrs_replay_step`, `cilrs_batch_assemble_view` and the
          forward, no host synchronisation, one read-back at the end;
  host    the same definition driven from the host through the public pieces: per tick
          `data.view_records` (+ `identity_view` for segments on the path), `DeviceDataset.assemble(
          view=)` (its `check_view` and its host-to-device copies), `model(...)`, a device-to-host
          copy of the controls and a vectorised float64 numpy step.

Both are timed by device events around the whole loop, alternated `--rounds` times in this one
process after a warm-up of each, at B = 128 and B = 1; min, median and max per tick are printed.
There is no pass threshold.  Writes profiles/replay_bench.log (--log).
Usage: python tools/replay_bench.py [--ticks 200] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd"))
H, W = 88, 200
BOX_M, BOX_DEG, DT = 1.0, 10.0, 0.05


def host_replay(model, ds, starts, ticks, lateral_m, yaw_deg, targets_host):
    """the loop of include/cilrs_hip.h ("closed-loop replay", no filter) from the host ->
    interventions per segment"""
    import numpy as np
    import torch
    from cilrs_mi355 import data as D
    b = len(starts)
    e, psi = np.full(b, float(lateral_m)), np.full(b, np.radians(yaw_deg))
    unit, wheel, base = D.SPEED_NORM_KMH / 3.6, np.radians(70.0), 2.875
    box_yaw = np.radians(BOX_DEG)
    params = D.identity_params(b)
    hits = np.zeros(b, dtype=np.int64)
    with torch.no_grad():
        for k in range(ticks):
            idx = starts + k
            v = ds.speed_host[idx].astype(np.float64)
            rec = D.view_records(e, psi, v, H, W)
            on_path = (e == 0.0) & (psi == 0.0)
            rec[on_path] = D.identity_view(int(on_path.sum()))
            img, spd, cmd, _tgt = ds.assemble(idx, params, view=rec)
            controls, _speed = model(img, spd, cmd)
            raw = controls[:, 0].cpu().numpy().astype(np.float64)
            bad = ~np.isfinite(raw)
            s = np.clip(np.where(bad, 0.0, raw), -1.0, 1.0)
            sx = np.clip(targets_host[idx, 0].astype(np.float64), -1.0, 1.0)
            step = v * unit * DT
            e2 = e + step * np.sin(psi)
            p2 = psi + step * (np.tan(s * wheel) - np.tan(sx * wheel)) / base
            out = bad | (np.abs(e2) > BOX_M) | (np.abs(p2) > box_yaw)
            hits += out
            e, psi = np.where(out, 0.0, e2), np.where(out, 0.0, p2)
    return hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default="128,1")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "replay_bench.log"),
                    help="the lines are written to this file too")
    args = ap.parse_args()

    import numpy as np
    import torch
    from cilrs_mi355 import CILRS
    from cilrs_mi355 import data as D
    from cilrs_mi355 import evaluate as E
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench: needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda")
    lines = []

    def log(m):
        print(m, flush=True)
        lines.append(m)

    g = torch.Generator().manual_seed(0)
    n, t = args.frames, args.ticks
    cache = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    speed = (0.1 + 0.9 * torch.rand(n, generator=g)).to(dev)
    command = torch.randint(0, 4, (n,), generator=g).to(dev)
    targets = torch.rand(n, 3, generator=g)
    targets[:, 0] = 0.2 * (targets[:, 0] * 2 - 1)
    ds = D.DeviceDataset.from_tensors(cache, speed, command, targets.to(dev))
    targets_host = targets.numpy()
    torch.manual_seed(0)
    model = CILRS(4, dropout=0.0).to(dev).eval()
    lat, yaw = 0.3, 2.0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / t, out                   # ms per tick

    res = {"device": torch.cuda.get_device_name(0), "frames": n, "ticks": t,
           "rounds": args.rounds}
    log(f"replay_bench: {res['device']}; {n} frames of {W}x{H}, T={t}, start ({lat} m, {yaw} deg), "
        f"box (+-{BOX_M} m, +-{BOX_DEG} deg), fp32 eval forward")
    for b in (int(v) for v in args.batches.split(",")):
        starts = np.random.default_rng(b).integers(0, n - t + 1, b)
        legs = {
            "device": lambda: sum(s["interventions"] for s in E.replay(
                model, ds, starts, t, lateral_m=lat, yaw_deg=yaw, dt=DT, max_lateral_m=BOX_M,
                max_yaw_deg=BOX_DEG, batch_size=b)["segments"]),
            "host": lambda: int(host_replay(model, ds, starts, t, lat, yaw, targets_host).sum())}
        for fn in legs.values():                             # warm-up: plans, code objects
            fn()
        ms = {k: [] for k in legs}
        hits = {}
        for r in range(args.rounds):
            for k, fn in legs.items():
                got, hits[k] = timed(fn)
                ms[k].append(round(got, 4))
            log(f"B={b} round {r}: " + ", ".join(f"{k} {ms[k][-1]:.4f}" for k in legs)
                + " ms per tick")
        for k in legs:
            v = ms[k]
            log(f"B={b} {k}: min {min(v):.4f}, median {float(np.median(v)):.4f}, max {max(v):.4f} "
                f"ms per tick; {hits[k]} interventions over {b * t} ticks")
        gain = float(np.median(ms["host"]) - np.median(ms["device"]))
        spread = max(ms["host"]) - min(ms["host"])
        log(f"B={b}: host - device = {gain:+.4f} ms per tick (medians); the host loop's own max - "
            f"min over the rounds is {spread:.4f} ms")
        res[f"b{b}"] = {"ms_per_tick": ms, "host_minus_device_ms": round(gain, 4),
                        "host_spread_ms": round(spread, 4), "interventions": hits}
    log(json.dumps(res))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
