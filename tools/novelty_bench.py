#!/usr/bin/env python3
"""What Predictor.predict_novelty adds to a control-loop tick, and FeatureDensity.update to a batch
of the fit.

Tick: B = 1, 88x200, for the ResNet-34 network (the persistent predictor) and the ResNet-50 variant
(F = 2048, per-layer launches), all in one process:
  (a) predict_batch                      the tick as it is
  (b) predict_novelty                    the tick + the three score launches + one more sync
  (c) the torch realisation a user could write without cilrs_net_novelty, timed alone, i.e. what
      it would ADD to (a): the pooled features from the plan's workspace (after the persistent
      launch: the mean of the stored map), W @ (v - mean[k]) and the squared norm with torch on
      the device, one synchronising copy
Fit: B = 128, 88x200: FeatureDensity.update against the bare eval-mode forward it contains.

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
import torch
import cilrs_oracle as O
from cilrs_mi355 import CILRS, CILRSResNet50
from cilrs_mi355.novelty import FeatureDensity
from cilrs_mi355.predict import Predictor
from cilrs_mi355 import _lib as L


def model(cls):
    m = cls(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
    return m.cuda().eval()


def torch_novelty(pred, pl, fd, k):
    """(c): W @ (v - mean[k]) and its squared norm with torch, on the plan's own features."""
    if pred.persistent:
        yo, zo, n, ch = L.sz(), L.sz(), L.sz(), L.i32()
        L.check(L.lib().cilrs_net_activation_info(pl.handle, 35, C.byref(yo), C.byref(zo), C.byref(n),
                                                  C.byref(ch)))
        fmap = pl.workspace.view(torch.float32)[zo.value:zo.value + n.value].view(-1, ch.value)
        features = lambda: fmap.mean(dim=0)
    else:
        comb = pred.eng.plan_features(pl)
        features = lambda: comb[0]
    W, mean = torch.tril(fd.W), fd.mean[k]
    out = torch.empty(1, dtype=torch.float32).pin_memory()

    @torch.no_grad()
    def run():
        y = W @ (features() - mean)
        out.copy_((y * y).sum().view(1), non_blocking=True)
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


def fit(m, batch, n_batches):
    """a density over n_batches synthetic batches (what the tick candidates score against)"""
    fd = FeatureDensity(m)
    for i in range(n_batches):
        img, spd, cmd, _t, _u8 = O.synthetic_batch(batch, seed=10 + i)
        fd.update(img.cuda(), spd.cuda(), cmd.cuda())
    return fd.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--fit-batch", type=int, default=128)
    ap.add_argument("--fit-calls", type=int, default=20)
    ap.add_argument("--fit-rounds", type=int, default=3)
    ap.add_argument("--networks", nargs="*", default=["resnet34", "resnet50"])
    args = ap.parse_args()
    u8 = O.synthetic_batch(1, seed=1)[4]
    kmh, cmd = [30.0], [2]
    for net in args.networks:
        m = model(CILRS if net == "resnet34" else CILRSResNet50)
        fd = fit(m, args.fit_batch, 3)
        pred = Predictor(m)
        pred.predict_batch(u8, kmh, cmd)
        pl = pred.eng.plan(1, 88, 200)
        cands = {
            "a_predict_batch": lambda: pred.predict_batch(u8, kmh, cmd),
            "b_predict_novelty": lambda: pred.predict_novelty(u8, kmh, cmd, fd),
            "c_torch_alone": torch_novelty(pred, pl, fd, cmd[0]),
        }
        r = measure(cands, args.calls, args.rounds, args.warmup)
        added = r["b_predict_novelty"]["ms"] - r["a_predict_batch"]["ms"]
        spread = max(v["spread"] for v in r.values())
        print(json.dumps({"config": f"tick B=1 88x200 {net} F={fd.F} "
                                    f"{'persistent' if pred.persistent else 'per-layer'}", **r,
                          "added_ms": round(added, 5),
                          "added_share_of_tick": round(added / r["a_predict_batch"]["ms"], 4),
                          "torch_minus_added_ms": round(r["c_torch_alone"]["ms"] - added, 5),
                          "largest_spread_ms": spread,
                          "added_beats_torch": bool(r["c_torch_alone"]["ms"] - added > spread)}),
              flush=True)
        # the fit: update() against the bare eval forward it contains
        img, spd, c, _t, _u8 = O.synthetic_batch(args.fit_batch, seed=3)
        img, spd, c = img.cuda(), spd.cuda(), c.cuda()
        fresh = FeatureDensity(m)

        def bare():
            with torch.no_grad():
                m(img, spd, c)
            torch.cuda.synchronize()

        def update():
            fresh.update(img, spd, c)
            torch.cuda.synchronize()
        r = measure({"forward": bare, "update": update}, args.fit_calls, args.fit_rounds, 3)
        added = r["update"]["ms"] - r["forward"]["ms"]
        print(json.dumps({"config": f"fit B={args.fit_batch} 88x200 {net} F={fd.F}", **r,
                          "added_ms": round(added, 5),
                          "added_share_of_update": round(added / r["update"]["ms"], 4),
                          "largest_spread_ms": max(v["spread"] for v in r.values())}), flush=True)


if __name__ == "__main__":
    main()
