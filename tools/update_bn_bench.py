#!/usr/bin/env python3
"""What one batch of BatchNorm re-estimation costs (BatchNormEstimator.update) beside the call it
is built from.

At B = 128, 88x200, variant 0, in one process:
  (a) Engine.run_forward(train=True)        the bare cilrs_net_forward(train = 1): trunk, heads,
                                            running buffers moved -- the nearest path without the
                                            estimator
  (b) BatchNormEstimator.update             cilrs_net_forward_bn_stats: the same trunk launches, no
                                            heads, the batch statistics added to the float64 table
and once, for the record, cilrs_bn_stats_finalize (one launch for the 36 layers; it reads 72
doubles back first, so host time is what is measured).

Device time between hipEvents around `--inner` back-to-back calls; both candidates warmed first;
they alternate inside each round; per candidate the median of each round's samples, over the
rounds the median of those and their max - min.  No speed-up is promised: (b) drops the heads and
adds one double chain per channel to launches that are latency-bound.  The difference is to be read
against the spread.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("cilrs-autonomous-driving-carla_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
import cilrs_oracle as O
from cilrs_mi355 import CILRS, BatchNormEstimator


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--height", type=int, default=88)
    ap.add_argument("--width", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    m = CILRS(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
    m = m.cuda().train()
    eng = m.engine()
    img, spd, cmd = (t.cuda() for t in O.synthetic_batch(a.batch, seed=1, h=a.height, w=a.width)[:3])
    est = BatchNormEstimator(m)
    cands = {"forward_train": lambda: eng.run_forward(img, spd, cmd, True, 0.0, 0),
             "estimator_update": lambda: est.update(img)}
    for fn in cands.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    per_round = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items():
            per_round[k].append(statistics.median(event_ms(fn, a.inner) for _ in range(a.samples)))
    out = {"what": "update_bn_bench", "batch": a.batch, "height": a.height, "width": a.width,
           "rounds": a.rounds, "samples": a.samples, "inner": a.inner,
           "device": torch.cuda.get_device_name(0)}
    for k, v in per_round.items():
        out[k] = {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4),
                  "per_round_ms": [round(x, 4) for x in v]}
    out["update_minus_forward_ms"] = round(out["estimator_update"]["median_ms"] -
                                           out["forward_train"]["median_ms"], 4)
    out["larger_spread_ms"] = max(out["estimator_update"]["spread_ms"],
                                  out["forward_train"]["spread_ms"])
    fin = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        est.finalize()
        torch.cuda.synchronize()
        fin.append((time.perf_counter() - t0) * 1e3)
    out["finalize_host_ms"] = {"median_ms": round(statistics.median(fin), 4),
                               "spread_ms": round(max(fin) - min(fin), 4)}
    out["batches_in_table"] = est.batches
    print(json.dumps(out))


if __name__ == "__main__":
    main()
