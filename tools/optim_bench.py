#!/usr/bin/env python3
"""What AdamW and LAMB (TrainConfig.optimizer) cost against the Adam step.

At the arena of variant 0 (22.4 M floats) with its real segment table (142 parameter tensors, the
1-D ones exempt), all in one process:
  (a) cilrs_adam_step                       7 arena-sized arrays moved, one launch
  (b) cilrs_optim_step, AdamW               7, one launch over the chunk table
  (c) cilrs_optim_step, LAMB                10 (p g m v -> m v; p m v -> p), three launches:
                                            moments + partial norms, finalise, apply
and at B = 128, 200x88, Config A, the whole train_step under each of the three optimizers.

Device time between hipEvents around `--inner` back-to-back calls (kernels) or `--steps` train
steps; every candidate warmed first; the candidates alternate inside each round; per candidate the
median of each round's samples, and over the rounds min / median / max of those.  One JSON line per
part."""
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
from cilrs_mi355.train import OPTIM_KIND, segment_table


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
    return {name: dict(min=round(min(v), 5), ms=round(statistics.median(v), 5), max=round(max(v), 5),
                       rounds=[round(x, 5) for x in v]) for name, v in per_round.items()}


def kernels(args):
    lib = L.lib()
    m = model()
    eng = m.engine()
    n, dev = eng.n_arena, eng.device
    p0 = eng.params.clone()
    g = torch.randn(n, device=dev) * 1e-3
    # padding floats are zero in every array
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    for _, off, numel, _ in eng.params_layout:
        keep[off:off + numel] = True
    g *= keep
    state = {k: (p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev))
             for k in ("adam", "adamw", "lamb")}
    tables = {}
    for name in ("adamw", "lamb"):
        ends, flags = segment_table(eng.params_layout, n, True, name == "lamb")
        k = len(ends)
        c_ends, c_flags = (C.c_size_t * k)(*ends), (C.c_int * k)(*flags)
        nbytes = lib.cilrs_optim_table_bytes(c_ends, k)
        mem = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        h = C.c_void_p()
        L.check(lib.cilrs_optim_table_create(c_ends, c_flags, k, n, L.ptr(mem), nbytes, None,
                                             C.byref(h)))
        scratch = torch.empty(max(lib.cilrs_optim_scratch_bytes(h), 16), dtype=torch.uint8, device=dev)
        tables[name] = (h, mem, scratch, torch.ones(k, device=dev), k, nbytes)
    step = {"adam": 0, "adamw": 0, "lamb": 0}

    def stream():
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def adam():
        step["adam"] += 1
        p, mom, var = state["adam"]
        L.check(lib.cilrs_adam_step(L.ptr(p), L.ptr(g), L.ptr(mom), L.ptr(var), n, 2e-4, 0.9, 0.999,
                                    1e-8, 1e-4, step["adam"], None, 1.0, stream()))

    def optim(name):
        h, _, scratch, ratios, k, _ = tables[name]
        p, mom, var = state[name]
        ends, lrs = (C.c_size_t * 1)(n), (C.c_double * 1)(2e-4)

        def fn():
            step[name] += 1
            L.check(lib.cilrs_optim_step(OPTIM_KIND[name], h, 0, k, L.ptr(p), L.ptr(g), L.ptr(mom),
                                         L.ptr(var), 1, ends, lrs, (C.c_int64 * 1)(step[name]), 0.9,
                                         0.999, 1e-8, 1e-4, 0.0, None, 1.0, L.ptr(scratch),
                                         L.ptr(ratios), stream()))
        return fn

    cands = {"a_adam": adam, "b_adamw": optim("adamw"), "c_lamb": optim("lamb")}
    r = measure(cands, args.samples, args.inner, args.rounds, args.warmup)
    a, b, c = (r[k]["ms"] for k in cands)
    arena_gb = n * 4 / 1e9
    ratios = tables["lamb"][3]
    print(json.dumps({
        "part": "kernels", "arena_floats": n, "segments": tables["lamb"][4],
        "chunks": tables["lamb"][5] // 16 - tables["lamb"][4], **r,
        "gbps": {"a": round(7 * arena_gb / a * 1e3, 1), "b": round(7 * arena_gb / b * 1e3, 1),
                 "c": round(10 * arena_gb / c * 1e3, 1)},
        "adamw_over_adam": round(b / a, 4), "lamb_over_adam": round(c / a, 4),
        "expected_by_arrays_moved": {"adamw_over_adam": 1.0, "lamb_over_adam": round(10 / 7, 4)},
        "lamb_ratio_range": [round(float(ratios.min()), 5), round(float(ratios.max()), 5)]}),
        flush=True)
    for h, *_ in tables.values():
        lib.cilrs_optim_table_destroy(h)


def steps(args):
    m = model()
    batch = [t.cuda() for t in O.synthetic_batch(args.batch, seed=1)[:4]]
    trs = {name: Trainer(m, TrainConfig(**{**CONFIG_A.__dict__, "optimizer": name,
                                           "decay_exempt_1d": name != "adam"}))
           for name in ("adam", "adamw", "lamb")}
    cands = {name: (lambda tr=tr: tr.train_step(*batch)) for name, tr in trs.items()}
    r = measure(cands, args.step_samples, args.steps, args.rounds, args.warmup)
    for tr in trs.values():
        tr.losses()                               # surfaces a bad status / non-finite loss
    base = r["adam"]["ms"]
    print(json.dumps({
        "part": "train_step", "batch": args.batch, "config": "A", **r,
        "steps_per_s": {k: round(1e3 / v["ms"], 2) for k, v in r.items()},
        "adamw_minus_adam_ms": round(r["adamw"]["ms"] - base, 5),
        "lamb_minus_adam_ms": round(r["lamb"]["ms"] - base, 5),
        "largest_spread_ms": round(max(v["max"] - v["min"] for v in r.values()), 5)}), flush=True)


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
    assert args.rounds >= 3, "min / median / max need at least three rounds"
    assert torch.cuda.is_available(), "optim_bench.py measures on the device; there is no CPU path"
    kernels(args)
    if not args.no_steps:
        steps(args)


if __name__ == "__main__":
    main()
