#!/usr/bin/env python3
"""What loss-prioritised sampling (PrioritySampler / PrioritizedBatchLoader) costs.

(a) At N = 176,256 table entries and B = 128: one cilrs_priority_draw (three launches) plus one
    cilrs_priority_update against the same definition written in torch on the device -- cumsum of
    the int64 table, the stratified targets from uniforms drawn beforehand (torch has no 64-bit
    high multiply, so the counter hash is left out of its side), searchsorted, the gather through
    the subset, the importance weights, pow and index_put_ (which does not settle repeated
    positions the way the kernel does).
(b) The fp32 B = 128, 200x88 Config A train step fed by CachedBatchLoader (the loader of the parent
    commit, unchanged) against the step fed by PrioritizedBatchLoader with alpha = 0.6, beta = 0.4:
    draw, assemble, the step with weights and row losses, the update.  Both over the same
    DeviceDataset of N random frames.

Device time between hipEvents; every candidate warmed first; the candidates alternate inside each
round; per candidate the median of a round's samples, over the rounds min / median / max of those.
One JSON line per part."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("cilrs-autonomous-driving-carla_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
import torch
import cilrs_oracle as O
from cilrs_mi355 import (CILRS, CONFIG_A, CachedBatchLoader, DeviceDataset, PrioritizedBatchLoader,
                         PrioritySampler, Trainer)


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def summary(per_round):
    return {name: dict(min=round(min(v), 5), ms=round(statistics.median(v), 5), max=round(max(v), 5),
                       rounds=[round(x, 5) for x in v]) for name, v in per_round.items()}


def kernels(args):
    n, B, dev = args.frames, args.batch, torch.device("cuda")
    rng = np.random.default_rng(0)
    base = (rng.random(n) + 0.5).astype(np.float32)
    subset = rng.permutation(n)
    s = PrioritySampler(n, dev, base=base, subset=subset, n_frames=n, alpha=0.6, beta=0.4, seed=1)
    loss = torch.rand(B, device=dev) * 2

    def ours():
        pos, _, _ = s.draw(B)
        s.update(pos, loss)

    def ours_draw():
        s.draw(B)

    q = torch.from_numpy(s.table().astype(np.int64)).to(dev)
    base_d, subset_d = torch.from_numpy(base).to(dev).double(), torch.from_numpy(subset).to(dev)
    u = torch.rand(B, device=dev, dtype=torch.float64)
    ar = torch.arange(B, device=dev)

    def torch_form():
        cum = torch.cumsum(q, 0)
        total = cum[-1]
        quo, rem = total // B, total % B
        lo = quo * ar + torch.minimum(ar, rem)
        ln = quo + (ar < rem)
        t = lo + (u * ln).long()
        pos = torch.searchsorted(cum, t, right=True)
        index = subset_d[pos]
        w = (total.double() / (n * q[pos].double())) ** 0.4
        w = (w / w.max()).float()
        p = base_d[pos] * (loss.double() + 1e-3) ** 0.6
        q.index_put_((pos,), torch.clamp(torch.round(p * 2.0 ** 20), 1, 2.0 ** 32 - 1).long())
        return index, w

    cands = {"a_draw_update": ours, "b_draw_only": ours_draw, "c_torch": torch_form}
    for fn in cands.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            per_round[name].append(statistics.median(event_ms(fn, args.inner)
                                                     for _ in range(args.samples)))
    r = summary(per_round)
    print(json.dumps({"part": "kernels", "n": n, "batch": B, **r,
                      "ours_over_torch": round(r["a_draw_update"]["ms"] / r["c_torch"]["ms"], 4),
                      "table_bytes": 4 * n}), flush=True)


def dataset(n, h=88, w=200):
    g = torch.Generator(device="cuda").manual_seed(0)
    cache = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda")
    for b0 in range(0, n, 8192):
        part = cache[b0:b0 + 8192]
        part.copy_(torch.randint(0, 256, part.shape, dtype=torch.uint8, device="cuda", generator=g))
    speed = torch.rand(n, device="cuda", generator=g)
    command = torch.randint(0, 4, (n,), device="cuda", generator=g)
    targets = torch.rand(n, 3, device="cuda", generator=g) * 2 - 1
    return DeviceDataset.from_tensors(cache, speed, command, targets)


def steps(args):
    ds = dataset(args.frames)
    idx = np.arange(args.frames)
    trs = {}
    for name in ("cached", "prioritised"):
        m = CILRS(4, 0.0)
        m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
        trs[name] = Trainer(m.cuda().train(), CONFIG_A)
    cached = iter(CachedBatchLoader(ds, idx, args.batch, True, seed=0))
    prio = PrioritizedBatchLoader(ds, idx, args.batch, seed=0, alpha=0.6, beta=0.4)
    prio_it = iter(prio)
    rows = torch.empty(args.batch, device="cuda")

    def cached_step():
        trs["cached"].train_step(*next(cached))

    def prio_step():
        batch = next(prio_it)
        trs["prioritised"].train_step(*batch, sample_weight=prio.last_weight, row_loss=rows)
        prio.feedback(rows)

    cands = {"cached": cached_step, "prioritised": prio_step}
    for fn in cands.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            per_round[name].append(statistics.median(event_ms(fn, args.steps)
                                                     for _ in range(args.step_samples)))
    for tr in trs.values():
        tr.losses()
    r = summary(per_round)
    print(json.dumps({
        "part": "train_step", "batch": args.batch, "frames": args.frames, "config": "A", **r,
        "prioritised_minus_cached_ms": round(r["prioritised"]["ms"] - r["cached"]["ms"], 5),
        "prioritised_over_cached": round(r["prioritised"]["ms"] / r["cached"]["ms"], 4),
        "largest_spread_ms": round(max(v["max"] - v["min"] for v in r.values()), 5),
        "draws": int(prio.sampler.counter), "running_max": prio.sampler.running_max(),
        "rows_calls": trs["prioritised"].rows_calls}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=176_256)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--samples", type=int, default=20, help="event windows per round (kernels)")
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per event window")
    ap.add_argument("--steps", type=int, default=30, help="train steps per event window")
    ap.add_argument("--step-samples", type=int, default=3, help="event windows per round (steps)")
    ap.add_argument("--no-steps", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "priority_bench.py measures on the device; there is no CPU path"
    assert args.rounds >= 3, "min / median / max need at least three rounds"
    kernels(args)
    if not args.no_steps:
        steps(args)


if __name__ == "__main__":
    main()
