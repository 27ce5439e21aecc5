#!/usr/bin/env python3
"""What weather on the device costs, at B=128, 88x200, on a device-resident dataset of random
frames.  Both sides of every comparison run in this one process, alternating, `--rounds` times after
a warm-up:

  (a) the launch alone, by device events, from records already on the device: the plain
      `cilrs_batch_assemble` against `cilrs_batch_assemble_weather` under the default `WeatherMix`
      and under all-`hardrain` -- the same training augmentation records on every side;
  (b) `CachedBatchLoader` feeding the fp32 and the bf16 train step, without and with the default mix.

There is no pass threshold.  Writes profiles/weather_bench.log (--log).
Usage: python tools/weather_bench.py [--frames 4096] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cilrs_mi355 import CILRS, CONFIG_A, Trainer  # noqa: E402
from cilrs_mi355 import data as D  # noqa: E402

H, W = D.IMG_HEIGHT, D.IMG_WIDTH


def measure(frames=4096, batch=128, rounds=3, launches=100, log=print):
    dev = torch.device("cuda")
    res = {"frames": frames, "batch": batch, "rounds": rounds, "launches": launches}
    g = torch.Generator().manual_seed(0)
    cache = torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    command = torch.from_numpy(np.random.default_rng(0).choice(
        4, frames, p=[0.5, 0.27, 0.14, 0.09]).astype(np.int64)).to(dev)
    ds = D.DeviceDataset.from_tensors(cache, torch.rand(frames, generator=g).to(dev), command,
                                      torch.rand(frames, 3, generator=g).to(dev))
    idx = np.arange(frames)

    # (a) the launch alone
    rng = np.random.default_rng(1)
    order = torch.from_numpy(rng.integers(0, frames, batch)).to(dev)
    up = lambda rec: torch.from_numpy(rec.view(np.uint8).reshape(batch, -1)).to(dev)
    params = D.draw_aug_params(np.random.default_rng(3), batch)
    pd = up(params)
    mixes = {"plain": None, "default_mix": D.WeatherMix(),
             "all_hardrain": D.WeatherMix({"hardrain": 1.0})}
    recs = {k: (None if m is None else m.draw(np.random.default_rng(4), batch, H, W))
            for k, m in mixes.items()}
    wd = {k: (None if r is None else up(r)) for k, r in recs.items()}
    res["blurred_samples"] = int((params["blur_k"] > 1).sum())
    for k, r in recs.items():
        if r is not None:
            res[f"{k}_rainy_samples"] = int((r["rain_len"] > 0).sum())
            res[f"{k}_weather_samples"] = int((r["tone_on"] == 1).sum())

    def launch_us(k):
        wp = None if wd[k] is None else wd[k].data_ptr()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            ds._launch(order.data_ptr(), pd.data_ptr(), batch, weather_ptr=wp)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches * 1e3

    for k in mixes:                               # warm-up
        launch_us(k)
        res[f"launch_us_{k}"] = []
    for r in range(rounds):
        for k in mixes:
            res[f"launch_us_{k}"].append(round(launch_us(k), 1))
        log(f"launch round {r}: " + ", ".join(f"{k} {res[f'launch_us_{k}'][-1]:.1f}" for k in mixes)
            + " us")

    # (b) the cached loader feeding the train step
    def epoch(batches, step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for img, spd, cmd, tgt in batches:
            step(img, spd, cmd, tgt)
            n += img.size(0)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    for prec in ("fp32", "bf16"):
        trainer = Trainer(CILRS(4, dropout=0.0).to(dev), CONFIG_A, precision=prec)
        legs = {"off": D.CachedBatchLoader(ds, idx, batch, train=True, seed=1),
                "mix": D.CachedBatchLoader(ds, idx, batch, train=True, seed=1,
                                           weather=D.WeatherMix())}
        for name, ld in legs.items():             # warm-up epoch of each leg
            epoch(ld, trainer.train_step)
            res[f"{prec}_{name}_frames_per_s"] = []
        for r in range(rounds):
            for name, ld in legs.items():
                res[f"{prec}_{name}_frames_per_s"].append(round(epoch(ld, trainer.train_step), 1))
            log(f"{prec} round {r}: " + ", ".join(
                f"weather {name} {res[f'{prec}_{name}_frames_per_s'][-1]:,.0f}" for name in legs)
                + " frames/s")
        off, mix = res[f"{prec}_off_frames_per_s"], res[f"{prec}_mix_frames_per_s"]
        ms = lambda v: batch / v * 1e3
        res[f"{prec}_step_ms_off"] = round(ms(np.median(off)), 4)
        res[f"{prec}_step_ms_mix"] = round(ms(np.median(mix)), 4)
        res[f"{prec}_off_spread_ms"] = round(ms(min(off)) - ms(max(off)), 4)
        log(f"{prec}: loader + step {res[f'{prec}_step_ms_off']:.3f} ms without, "
            f"{res[f'{prec}_step_ms_mix']:.3f} ms with the mix (medians); the weather-off side's own "
            f"max-min over the rounds is {res[f'{prec}_off_spread_ms']:.3f} ms")
        del trainer
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "weather_bench.log"),
                    help="the lines are written to this file too")
    args = ap.parse_args()
    lines = []

    def log(m):
        print(m, flush=True)
        lines.append(m)
    log(f"weather_bench: {torch.cuda.get_device_name(0)}")
    res = measure(args.frames, args.batch, args.rounds, log=log)
    log(json.dumps(res))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
