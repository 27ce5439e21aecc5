#!/usr/bin/env python3
"""What the EMA of the weights (TrainConfig.ema_decay) adds to the optimizer step.

At the arena size of variant 0 (22.4 M floats), all in one process:
  (a) cilrs_adam_step                                 7 arena-sized arrays moved
  (b) cilrs_adam_step_ema                             9: the average fused into the Adam launch
  (c) cilrs_adam_step, then cilrs_ema_update          10, and one more launch
  (d) cilrs_adam_step, then torch._foreach_lerp_ over the 142 parameter views -- what a user could
      write without the library's help (not the same rounding as the definition; timing only)
and at B = 128, 200x88, Config A, the whole train_step:
  EMA off / EMA on through (c) (Trainer.ema_fused = False, the default) / EMA on, fused
  (Trainer.ema_fused = True); both routes are set explicitly, whatever the default is

Device time between hipEvents around `--inner` back-to-back calls (kernels) or `--steps` train
steps; every candidate warmed first; the candidates alternate inside each round; per candidate the
median of each round's samples, and over the rounds the median of those and their max - min.  The
fused route stays the Trainer's default only if (b) beats (c) by more than the larger of their
spreads.  One JSON line per part."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("cilrs-autonomous-driving-carla_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
import cilrs_oracle as O
from cilrs_mi355 import CILRS, CONFIG_A, TrainConfig, Trainer
from cilrs_mi355 import _lib as L
from cilrs_mi355.engine import _arena_view


def model():
    m = CILRS(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
    return m.cuda().train()


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def measure(cands, samples, inner, rounds, warmup):
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    per_round = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            per_round[name].append(statistics.median(event_ms(fn, inner) for _ in range(samples)))
    return {name: dict(ms=round(statistics.median(v), 5), spread=round(max(v) - min(v), 5),
                       rounds=[round(x, 5) for x in v]) for name, v in per_round.items()}


def kernels(args):
    lib = L.lib()
    m = model()
    eng = m.engine()
    n = eng.n_arena
    dev = eng.device
    p = eng.params.clone()
    g = torch.randn(n, device=dev) * 1e-3
    mom, var = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ema = p.clone()
    w = C.c_float(1.0 - 0.999).value
    views = [_arena_view(p, off, numel, shape) for _, off, numel, shape in eng.params_layout]
    ema_views = [_arena_view(ema, off, numel, shape) for _, off, numel, shape in eng.params_layout]
    step = [0]

    def stream():
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def adam():
        step[0] += 1
        L.check(lib.cilrs_adam_step(L.ptr(p), L.ptr(g), L.ptr(mom), L.ptr(var), n, 2e-4, 0.9, 0.999,
                                    1e-8, 1e-4, step[0], None, 1.0, stream()))

    def adam_ema():
        step[0] += 1
        L.check(lib.cilrs_adam_step_ema(L.ptr(p), L.ptr(g), L.ptr(mom), L.ptr(var), n, 2e-4, 0.9,
                                        0.999, 1e-8, 1e-4, step[0], None, 1.0, L.ptr(ema), w,
                                        stream()))

    def adam_then_ema():
        adam()
        L.check(lib.cilrs_ema_update(L.ptr(ema), L.ptr(p), n, w, stream()))

    def adam_then_foreach():
        adam()
        torch._foreach_lerp_(ema_views, views, w)

    cands = {"a_adam": adam, "b_adam_ema_fused": adam_ema, "c_adam_then_ema_update": adam_then_ema,
             "d_adam_then_torch_foreach": adam_then_foreach}
    r = measure(cands, args.samples, args.inner, args.rounds, args.warmup)
    a, b, c, d = (r[k]["ms"] for k in cands)
    spread = max(r["b_adam_ema_fused"]["spread"], r["c_adam_then_ema_update"]["spread"])
    arena_gb = n * 4 / 1e9
    print(json.dumps({
        "part": "kernels", "arena_floats": n, **r,
        "gbps": {"a": round(7 * arena_gb / a * 1e3, 1), "b": round(9 * arena_gb / b * 1e3, 1),
                 "c": round(10 * arena_gb / c * 1e3, 1)},
        "b_minus_a_ms": round(b - a, 5), "c_minus_a_ms": round(c - a, 5),
        "d_minus_a_ms": round(d - a, 5),
        "b_minus_a_over_a": round((b - a) / a, 4), "c_minus_a_over_a": round((c - a) / a, 4),
        "expected_by_bytes": {"b_minus_a_over_a": round(2 / 7, 4), "c_minus_a_over_a": round(3 / 7, 4)},
        "c_minus_b_ms": round(c - b, 5), "larger_spread_b_c_ms": spread,
        "fused_beats_separate": bool(c - b > spread)}), flush=True)


def steps(args):
    m = model()
    batch = [t.cuda() for t in O.synthetic_batch(args.batch, seed=1)[:4]]
    on = TrainConfig(**{**CONFIG_A.__dict__, "ema_decay": 0.999})
    trs = {"ema_off": Trainer(m, CONFIG_A), "ema_fused": Trainer(m, on), "ema_separate": Trainer(m, on)}
    trs["ema_fused"].ema_fused = True
    trs["ema_separate"].ema_fused = False
    assert trs["ema_off"].ema is None
    cands = {name: (lambda tr=tr: tr.train_step(*batch)) for name, tr in trs.items()}
    r = measure(cands, args.step_samples, args.steps, args.rounds, args.warmup)
    for tr in trs.values():
        tr.losses()                               # surfaces a bad status / non-finite loss
    off = r["ema_off"]["ms"]
    print(json.dumps({
        "part": "train_step", "batch": args.batch, "config": "A", **r,
        "steps_per_s": {k: round(1e3 / v["ms"], 2) for k, v in r.items()},
        "fused_minus_off_ms": round(r["ema_fused"]["ms"] - off, 5),
        "separate_minus_off_ms": round(r["ema_separate"]["ms"] - off, 5),
        "largest_spread_ms": max(v["spread"] for v in r.values())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--samples", type=int, default=20, help="event windows per round (kernels)")
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per event window")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=30, help="train steps per event window")
    ap.add_argument("--step-samples", type=int, default=3, help="event windows per round (steps)")
    ap.add_argument("--no-steps", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ema_bench.py measures on the device; there is no CPU path"
    kernels(args)
    if not args.no_steps:
        steps(args)


if __name__ == "__main__":
    main()
