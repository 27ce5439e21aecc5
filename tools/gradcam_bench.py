#!/usr/bin/env python3
"""What Predictor.gradcam adds to a control-loop tick.

At B = 1, 88x200, the persistent predictor, all in one process:
  (a) predict_batch                      the tick as it is
  (b) gradcam(layer="layer4")            the tick + the heads' input gradient + the map launch + one
                                         more synchronise
  (c) gradcam(layer="layer3")            the graph-keeping forward, two segments of the data-gradient
                                         chain, the map launch
  (d) saliency                           what a user has today: the graph-keeping forward and the
                                         whole data-gradient chain down to the stem

Host wall-clock around calls that end in a synchronise; every candidate warmed first; the candidates
alternate inside each round; per candidate the median of each round's calls, and over the rounds
the median of those and their max - min.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("cilrs-autonomous-driving-carla_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import cilrs_oracle as O
from cilrs_mi355 import CILRS
from cilrs_mi355.predict import Predictor


def model():
    m = CILRS(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
    return m.cuda().eval()


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
    args = ap.parse_args()
    pred = Predictor(model())
    assert pred.persistent
    u8 = O.synthetic_batch(1, seed=1)[4]
    kmh, cmd = [30.0], [2]
    cands = {
        "a_predict_batch": lambda: pred.predict_batch(u8, kmh, cmd),
        "b_gradcam_layer4": lambda: pred.gradcam(u8, kmh, cmd, layer="layer4"),
        "c_gradcam_layer3": lambda: pred.gradcam(u8, kmh, cmd, layer="layer3"),
        "d_saliency": lambda: pred.saliency(u8, kmh, cmd),
    }
    r = measure(cands, args.calls, args.rounds, args.warmup)
    a = r["a_predict_batch"]["ms"]
    added_b = r["b_gradcam_layer4"]["ms"] - a
    added_c = r["c_gradcam_layer3"]["ms"] - a
    added_d = r["d_saliency"]["ms"] - a
    spread = max(v["spread"] for v in r.values())
    print(json.dumps({"config": "B=1 88x200 persistent", **r,
                      "layer4_added_ms": round(added_b, 5),
                      "layer4_added_share_of_tick": round(added_b / a, 4),
                      "layer3_added_ms": round(added_c, 5),
                      "saliency_added_ms": round(added_d, 5),
                      "saliency_minus_layer4_added_ms": round(added_d - added_b, 5),
                      "largest_spread_ms": spread,
                      "layer4_beats_saliency": bool(added_d - added_b > spread),
                      "layer4_added_below_the_tick": bool(added_b < a)}), flush=True)


if __name__ == "__main__":
    main()
