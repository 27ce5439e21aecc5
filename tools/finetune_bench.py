#!/usr/bin/env python3
"""Fine-tuning step time per cut: ms per fused train step at B=128, 200x88, Config A with the
first k trunk groups frozen (CILRS.freeze), k = 0..5, all in one process.

  finetune_bench.py                  the table: k, ms/step, speed-up over k = 0
  finetune_bench.py --lr-mult        k = 0 with and without an all-distinct TrainConfig.lr_mult
                                     (five extra Adam range launches per step), alternating
  finetune_bench.py --fold-ab        the frozen prefix's convolutions per layer shape, Winograd
                                     kernel with the folded epilogue against the implicit-GEMM
                                     eval launch it replaces: needs an experiments build
                                     (tools/exp_build.sh, CILRS_LIB=tools/bin/libcilrs_hip_exp.so),
                                     where CILRS_FT_WINO=0 puts the implicit GEMM back

Device time between hipEvents around `--steps` steps after `--warmup` steps; one JSON line each."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("cilrs-autonomous-driving-carla_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
import cilrs_oracle as O
from cilrs_mi355 import CILRS, CONFIG_A, TrainConfig, Trainer

GROUPS = ("stem", "layer1", "layer2", "layer3", "layer4")


def model():
    m = CILRS(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
    return m.cuda().train()


def timed_steps(tr, batch, steps, warmup):
    for _ in range(warmup):
        tr.train_step(*batch)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.train_step(*batch)
    e1.record()
    torch.cuda.synchronize()
    tr.losses()                               # surfaces a bad status / non-finite loss
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lr-mult", action="store_true")
    ap.add_argument("--fold-ab", action="store_true")
    args = ap.parse_args()
    batch = [t.cuda() for t in O.synthetic_batch(args.batch, seed=1)[:4]]
    if args.lr_mult:
        mult = {"stem": 0.01, "layer1": 0.03, "layer2": 0.1, "layer3": 0.2, "layer4": 0.5, "heads": 1.0}
        trs = {"plain": Trainer(model(), CONFIG_A),
               "lr_mult": Trainer(model(), TrainConfig(**{**CONFIG_A.__dict__, "lr_mult": mult}))}
        out = {name: [] for name in trs}
        for _ in range(args.repeats):
            for name, tr in trs.items():
                out[name].append(round(timed_steps(tr, batch, args.steps, args.warmup), 4))
        print(json.dumps({"metric": "k=0 step, ms", "batch": args.batch, **out}))
        return
    if args.fold_ab:
        m = model()
        tr = Trainer(m, CONFIG_A)
        m.freeze("layer3")
        pl = tr.eng.plan(args.batch, batch[0].size(2), batch[0].size(3))
        res = {}
        for rep in range(args.repeats):
            for mode in ("1", "0"):
                os.environ["CILRS_FT_WINO"] = mode
                m.weights_changed()           # the prefix's cached state is rebuilt for this mode
                for _ in range(args.warmup):
                    tr.train_step(*batch)
                pl.profile(True)
                pl.profile_reset()
                for _ in range(args.steps):
                    tr.train_step(*batch)
                torch.cuda.synchronize()
                rows = pl.profile_table()
                pl.profile(False)
                launches = pl.ft_wino_convs()
                for grp in ("layer1", "layer2", "layer3"):
                    r = rows["conv_fwd." + grp]
                    res.setdefault(grp, {}).setdefault("wino_fold" if mode == "1" else "igemm", []).append(
                        round(r["ms"] / args.steps, 4))
                res.setdefault("fold_launches", {})[mode] = launches
        print(json.dumps({"metric": "frozen conv_fwd per group, ms per step (serialised, profiled)",
                          "batch": args.batch, **res}))
        return
    m = model()
    tr = Trainer(m, CONFIG_A)
    table = {k: [] for k in range(6)}
    for _ in range(args.repeats):
        for k in range(6):
            m.unfreeze()
            if k:
                m.freeze(GROUPS[k - 1])
            table[k].append(round(timed_steps(tr, batch, args.steps, args.warmup), 4))
    base = sum(table[0]) / len(table[0])
    for k in range(6):
        mean = sum(table[k]) / len(table[k])
        print(json.dumps({"k": k, "frozen": list(GROUPS[:k]), "ms_per_step": table[k],
                          "mean_ms": round(mean, 4), "speedup_vs_k0": round(base / mean, 3)}))


if __name__ == "__main__":
    main()
