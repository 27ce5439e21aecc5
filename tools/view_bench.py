#!/usr/bin/env python3
"""What the viewpoint warp costs, at B=128, 88x200, on a device-resident cache of random frames.

  (a) the assemble launch alone, by device events, from records already on the device, in five
      modes: plain (`cilrs_batch_assemble`), weather (`_weather`, default `WeatherMix`), view
      (`cilrs_batch_assemble_view`, default `ViewShift`, no weather), view + weather, and
      view + weather with every sample warped and blurred 5x5 (25 taps of 4 source reads each) --
      the same training augmentation records otherwise.  Every round is a fresh child process per
      library, this tree's and (--parent-lib, a build of the parent commit) the parent's, alternated
      `--rounds` times in this one run; the parent's library has the first two modes only.  The
      children call the C entry points through ctypes directly, the same way on both sides.
  (b) `CachedBatchLoader` feeding the fp32 and the bf16 train step, without and with the default
      `ViewShift`, alternated in one process.

There is no pass threshold.  Writes profiles/view_bench.log (--log).
Usage: python tools/view_bench.py [--parent-lib tools/bin/libcilrs_hip_parent.so] [--rounds 3]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd")
sys.path.insert(0, PKG)
TREE_LIB = os.path.join(PKG, "cilrs_mi355", "libcilrs_hip.so")
MODES = ("plain", "weather", "view", "view_weather", "view_weather_blur5")
PARENT_MODES = MODES[:2]
H, W = 88, 200


def launch_child(lib_path, modes, frames, batch, launches):
    """us per launch of every mode, through `lib_path`; prints one JSON line"""
    import numpy as np
    import torch
    from cilrs_mi355 import data as D
    dev = torch.device("cuda")
    lib = C.CDLL(lib_path)
    g = torch.Generator().manual_seed(0)
    cache = torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    speed_host = torch.rand(frames, generator=g)
    speed = speed_host.to(dev)
    command = torch.randint(0, 4, (frames,), generator=g).to(dev)
    targets = torch.rand(frames, 3, generator=g).to(dev)
    order_host = np.random.default_rng(1).integers(0, frames, batch)
    order = torch.from_numpy(order_host).to(dev)
    up = lambda rec: torch.from_numpy(rec.view(np.uint8).reshape(batch, -1)).to(dev)
    params = D.draw_aug_params(np.random.default_rng(3), batch)
    weather = D.WeatherMix().draw(np.random.default_rng(4), batch, H, W)
    spd = speed_host.numpy()[order_host]
    view = D.ViewShift().draw(np.random.default_rng(5), batch, spd, H, W)
    every = D.ViewShift(p=1.0).draw(np.random.default_rng(5), batch, spd, H, W)
    blur5 = params.copy()
    blur5["blur_k"], blur5["blur_w"] = 5, D.gaussian_taps(5, 1.5)
    D.check_view(view, H, W)
    D.check_view(every, H, W)
    pd, p5, wd, vd, ed = up(params), up(blur5), up(weather), up(view), up(every)
    out = torch.empty(batch, H, W, 3, dtype=torch.float32, device=dev)
    ospd = torch.empty(batch, dtype=torch.float32, device=dev)
    ocmd = torch.empty(batch, dtype=torch.int64, device=dev)
    otgt = torch.empty(batch, 3, dtype=torch.float32, device=dev)
    vp = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = (vp(cache), C.c_int64(frames), vp(speed), vp(command), vp(targets), vp(order))
    tail = (C.c_int(batch), C.c_int(H), C.c_int(W), vp(out), vp(None), vp(ospd), vp(ocmd), vp(otgt),
            stream)
    calls = {
        "plain": lambda: lib.cilrs_batch_assemble(*head, vp(pd), *tail),
        "weather": lambda: lib.cilrs_batch_assemble_weather(*head, vp(pd), vp(wd), *tail),
        "view": lambda: lib.cilrs_batch_assemble_view(*head, vp(pd), vp(None), vp(vd), *tail),
        "view_weather": lambda: lib.cilrs_batch_assemble_view(*head, vp(pd), vp(wd), vp(vd), *tail),
        "view_weather_blur5": lambda: lib.cilrs_batch_assemble_view(*head, vp(p5), vp(wd), vp(ed),
                                                                    *tail)}
    res = {"device": torch.cuda.get_device_name(0), "view_on_samples": int((view["on"] == 1).sum()),
           "blurred_samples": int((params["blur_k"] > 1).sum()),
           "weather_samples": int((weather["tone_on"] == 1).sum())}
    for k in modes:
        call = calls[k]
        for _ in range(10):                                  # warm-up
            if call() != 0:
                raise RuntimeError(f"{k}: the entry point refused the call")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        res[k] = round(e0.elapsed_time(e1) / launches * 1e3, 1)
    print(json.dumps(res), flush=True)


def step_child(frames, batch, rounds):
    """loader + train step without and with the default ViewShift; prints one JSON line"""
    import numpy as np
    import torch
    from cilrs_mi355 import CILRS, CONFIG_A, Trainer
    from cilrs_mi355 import data as D
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    cache = torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    command = torch.from_numpy(np.random.default_rng(0).choice(
        4, frames, p=[0.5, 0.27, 0.14, 0.09]).astype(np.int64)).to(dev)
    ds = D.DeviceDataset.from_tensors(cache, torch.rand(frames, generator=g).to(dev), command,
                                      torch.rand(frames, 3, generator=g).to(dev))
    idx = np.arange(frames)

    def epoch(batches, step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for img, spd, cmd, tgt in batches:
            step(img, spd, cmd, tgt)
            n += img.size(0)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    res = {}
    ms = lambda v: batch / v * 1e3
    for prec in ("fp32", "bf16"):
        trainer = Trainer(CILRS(4, dropout=0.0).to(dev), CONFIG_A, precision=prec)
        legs = {"off": D.CachedBatchLoader(ds, idx, batch, train=True, seed=1),
                "view": D.CachedBatchLoader(ds, idx, batch, train=True, seed=1,
                                            view=D.ViewShift())}
        fps = {name: [] for name in legs}
        for name, ld in legs.items():                        # warm-up epoch of each leg
            epoch(ld, trainer.train_step)
        for _ in range(rounds):
            for name, ld in legs.items():
                fps[name].append(round(epoch(ld, trainer.train_step), 1))
        for name in legs:
            res[f"{prec}_{name}_frames_per_s"] = fps[name]
            res[f"{prec}_step_ms_{name}"] = round(ms(np.median(fps[name])), 4)
        res[f"{prec}_off_spread_ms"] = round(ms(min(fps["off"])) - ms(max(fps["off"])), 4)
        del trainer
    print(json.dumps(res), flush=True)


def child(args, extra):
    """one fresh process; -> its JSON line"""
    cmd = [sys.executable, os.path.abspath(__file__), "--frames", str(args.frames), "--batch",
           str(args.batch), "--rounds", str(args.rounds), "--launches", str(args.launches)] + extra
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True,
                         timeout=args.child_timeout).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--parent-lib", default=None,
                    help="libcilrs_hip.so built from the parent commit (plain and weather modes)")
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "view_bench.log"),
                    help="the lines are written to this file too")
    ap.add_argument("--launch-child", default=None, metavar="LIB", help=argparse.SUPPRESS)
    ap.add_argument("--modes", default=",".join(MODES), help=argparse.SUPPRESS)
    ap.add_argument("--step-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.launch_child:
        return launch_child(args.launch_child, args.modes.split(","), args.frames, args.batch,
                            args.launches)
    if args.step_child:
        return step_child(args.frames, args.batch, args.rounds)

    import numpy as np
    lines = []

    def log(m):
        print(m, flush=True)
        lines.append(m)
    sides = [("tree", TREE_LIB, MODES)]
    if args.parent_lib:
        sides.append(("parent", os.path.abspath(args.parent_lib), PARENT_MODES))
    us = {side: {k: [] for k in modes} for side, _, modes in sides}
    info = None
    for r in range(args.rounds):
        for side, path, modes in sides:
            got = child(args, ["--launch-child", path, "--modes", ",".join(modes)])
            info = info or got
            for k in modes:
                us[side][k].append(got[k])
            log(f"launch round {r} {side}: " + ", ".join(f"{k} {got[k]:.1f}" for k in modes) + " us")
    log(f"view_bench: {info['device']}; B={args.batch}: {info['view_on_samples']} samples warped "
        f"under the default ViewShift, {info['weather_samples']} under weather, "
        f"{info['blurred_samples']} blurred (view_weather_blur5: every sample warped and blurred 5x5)")
    res = {"frames": args.frames, "batch": args.batch, "rounds": args.rounds,
           "launches": args.launches, "launch_us": us}
    for k in MODES:
        res[f"launch_us_{k}"] = float(np.median(us["tree"][k]))
        log(f"{k}: {res[f'launch_us_{k}']:.1f} us per launch (median of {args.rounds})")
    if args.parent_lib:
        for k in PARENT_MODES:
            d = float(np.median(us["tree"][k]) - np.median(us["parent"][k]))
            spread = float(max(us["parent"][k]) - min(us["parent"][k]))
            res[f"{k}_tree_minus_parent_us"], res[f"{k}_parent_spread_us"] = round(d, 1), round(spread, 1)
            log(f"{k}: tree - parent = {d:+.1f} us (medians); the parent's own max - min over the "
                f"rounds is {spread:.1f} us")
    step = child(args, ["--step-child"])
    res.update(step)
    for prec in ("fp32", "bf16"):
        off, view = step[f"{prec}_step_ms_off"], step[f"{prec}_step_ms_view"]
        log(f"{prec}: loader + step {off:.3f} ms without, {view:.3f} ms with the default ViewShift "
            f"(medians, {view - off:+.3f} ms = {100 * (view - off) / off:+.2f} % of the step); the "
            f"view-off side's own max - min over the rounds is {step[f'{prec}_off_spread_ms']:.3f} ms")
    log(json.dumps(res))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
