#!/usr/bin/env python3
"""What Predictor.predict_uncertain adds to a control-loop tick.

At B = 1, 88x200, the persistent predictor and S in {8, 32, 128}, all in one process:
  (a) predict_batch                               the tick as it is
  (b) predict_uncertain(samples=S)                the tick + the MC-dropout launches + one more sync
  (c) the torch realisation a user could write without cilrs_net_heads_mc: the module's own
      nn.Sequential heads on the device, Dropout in train mode, on S copies of the average of the
      feature map the plan stored, mean / std on the device, one synchronising copy -- timed alone,
      i.e. what it would ADD to (a)
and, for the record, (a) / (b) at B = 64 with the fp16 trunk and S = 32.

Host wall-clock around calls that end in a synchronise; every shape warmed first; the candidates
alternate inside each round; per candidate the median of each round's calls, and over the rounds
the median of those and their max - min.  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("cilrs-autonomous-driving-carla_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
import torch
import cilrs_oracle as O
from cilrs_mi355 import CILRS
from cilrs_mi355.predict import Predictor
from cilrs_mi355 import _lib as L


def model():
    m = CILRS(4, 0.5)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
    return m.cuda().eval()


def torch_heads_mc(m, pl, speed, k, S):
    """(c): train-mode nn.Sequential heads on S copies of the plan's pooled features."""
    yo, zo, n, ch = L.sz(), L.sz(), L.sz(), L.i32()
    L.check(L.lib().cilrs_net_activation_info(pl.handle, 35, C.byref(yo), C.byref(zo), C.byref(n),
                                              C.byref(ch)))
    fmap = pl.workspace.view(torch.float32)[zo.value:zo.value + n.value].view(-1, ch.value)
    heads = (m.speed_encoder, m.control_branches[k], m.speed_predictor)
    for h in heads:
        h.train()
    out = torch.empty(2, 4, dtype=torch.float32).pin_memory()

    @torch.no_grad()
    def run():
        v = fmap.mean(dim=0, keepdim=True).expand(S, -1)
        f = heads[0](speed.view(1, 1).expand(S, 1))
        c = heads[1](torch.cat([v, f], dim=1))
        x = torch.cat([c, heads[2](v)], dim=1)
        out.copy_(torch.stack([x.mean(dim=0), x.std(dim=0)]), non_blocking=True)
        torch.cuda.synchronize()
        return out
    return run


def measure(cands, calls, rounds, warmup):
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    per_round = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            ts = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            per_round[name].append(statistics.median(ts) * 1e3)
    return {name: dict(ms=round(statistics.median(v), 5), spread=round(max(v) - min(v), 5),
                       rounds=[round(x, 5) for x in v]) for name, v in per_round.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--samples", type=int, nargs="*", default=[8, 32, 128])
    ap.add_argument("--no-batch64", action="store_true")
    args = ap.parse_args()
    m = model()
    pred = Predictor(m)
    assert pred.persistent
    u8 = O.synthetic_batch(1, seed=1)[4]
    kmh, cmd = [30.0], [2]
    pred.predict_batch(u8, kmh, cmd)
    pl = pred.eng.plan(1, 88, 200)
    speed_d = torch.tensor([30.0 / 90.0], dtype=torch.float32, device="cuda")
    for S in args.samples:
        cands = {
            "a_predict_batch": lambda: pred.predict_batch(u8, kmh, cmd),
            "b_predict_uncertain": lambda S=S: pred.predict_uncertain(u8, kmh, cmd, samples=S),
            "c_torch_heads_alone": torch_heads_mc(m, pl, speed_d, cmd[0], S),
        }
        r = measure(cands, args.calls, args.rounds, args.warmup)
        added = r["b_predict_uncertain"]["ms"] - r["a_predict_batch"]["ms"]
        spread = max(r["b_predict_uncertain"]["spread"], r["a_predict_batch"]["spread"],
                     r["c_torch_heads_alone"]["spread"])
        print(json.dumps({"config": "B=1 88x200 persistent", "samples": S, **r,
                          "added_ms": round(added, 5),
                          "added_share_of_tick": round(added / r["a_predict_batch"]["ms"], 4),
                          "torch_minus_added_ms": round(r["c_torch_heads_alone"]["ms"] - added, 5),
                          "largest_spread_ms": spread,
                          "added_beats_torch": bool(r["c_torch_heads_alone"]["ms"] - added > spread)}),
              flush=True)
    if not args.no_batch64:
        pred64 = Predictor(m, batch=64, half=True)
        u8b = O.synthetic_batch(64, seed=2)[4]
        kmhb, cmdb = list(np.linspace(5.0, 80.0, 64)), [i % 4 for i in range(64)]
        cands = {"a_predict_batch": lambda: pred64.predict_batch(u8b, kmhb, cmdb),
                 "b_predict_uncertain": lambda: pred64.predict_uncertain(u8b, kmhb, cmdb, samples=32)}
        r = measure(cands, max(args.calls // 3, 20), args.rounds, 10)
        print(json.dumps({"config": "B=64 88x200 fp16 trunk (for the record)", "samples": 32, **r,
                          "added_ms": round(r["b_predict_uncertain"]["ms"] - r["a_predict_batch"]["ms"], 5)}),
              flush=True)


if __name__ == "__main__":
    main()
