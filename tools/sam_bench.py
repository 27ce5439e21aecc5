#!/usr/bin/env python3
"""What sharpness-aware minimisation (TrainConfig.sam_rho) costs.

(a) Over the arena of variant 0 (22.4 M floats), in one process: the three launches of
    cilrs_sam_perturb plus cilrs_sam_restore, plain and adaptive, against the same arithmetic in
    torch on the flat arena -- g.norm() in double, backup.copy_(p), p.add_(g, alpha=s),
    p.copy_(backup).  By arrays moved: perturb 5 (p g; p g -> backup p), 6 adaptive (the norm pass
    reads p too), restore 2; Adam moves 7.
(b) The B = 128, 200x88 Config A train_step: plain, SAM (sam_every=1) and sam_every=2 of this tree,
    and -- with --parent DIR, a built checkout of the parent commit -- the parent's plain step, measured
    by a child process per round (one library per process) between this tree's candidates.

Device time between hipEvents around `--inner` back-to-back calls (kernels) or `--steps` train
steps; every candidate warmed first; the candidates alternate inside each round; per candidate the
median of each round's samples, and over the rounds min / median / max of those.  One JSON line per
part."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree_arg():
    """--tree DIR has to be known before the package is imported"""
    for i, a in enumerate(sys.argv):
        if a == "--tree" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
    return ROOT


TREE = _tree_arg()
for p in ("cilrs-autonomous-driving-carla_amd", "oracle"):
    sys.path.insert(0, os.path.join(TREE, p))
import torch
import cilrs_oracle as O
from cilrs_mi355 import CILRS, CONFIG_A, TrainConfig, Trainer
from cilrs_mi355 import _lib as L


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


def warm(cands, warmup):
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()


def summary(per_round):
    return {name: dict(min=round(min(v), 5), ms=round(statistics.median(v), 5), max=round(max(v), 5),
                       rounds=[round(x, 5) for x in v]) for name, v in per_round.items()}


def kernels(args):
    lib = L.lib()
    eng = model().engine()
    n, dev = eng.n_arena, eng.device
    g = torch.randn(n, device=dev) * 1e-3
    state = {k: eng.params.clone() for k in ("sam", "asam", "torch")}
    backup = torch.empty(n, device=dev)
    scratch = torch.zeros(lib.cilrs_sam_scratch_bytes(n) // 8, dtype=torch.float64, device=dev)
    out3 = scratch[-3:]
    rho = 0.05

    def stream():
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def ours(name, adaptive):
        p = state[name]

        def fn():
            L.check(lib.cilrs_sam_perturb(L.ptr(p), L.ptr(g), L.ptr(backup), n, rho, adaptive,
                                          L.ptr(scratch), L.ptr(out3), stream()))
            L.check(lib.cilrs_sam_restore(L.ptr(p), L.ptr(backup), n, stream()))
        return fn

    tbackup = torch.empty(n, device=dev)

    def torch_form():
        p = state["torch"]
        s = rho / (g.norm(dtype=torch.float64) + 1e-12)        # stays on the device
        tbackup.copy_(p)
        p.add_(g * s.float())          # (add_(g, alpha=) takes a host number: that would synchronise)
        p.copy_(tbackup)

    def torch_alpha():
        p = state["torch"]
        s = float(rho / (g.norm(dtype=torch.float64) + 1e-12))   # the issue's form: one host read
        tbackup.copy_(p)
        p.add_(g, alpha=s)
        p.copy_(tbackup)

    cands = {"a_sam": ours("sam", 0), "b_asam": ours("asam", 1), "c_torch_device_scalar": torch_form,
             "d_torch_alpha_host_scalar": torch_alpha}
    warm(cands, args.warmup)
    per_round = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            per_round[name].append(statistics.median(event_ms(fn, args.inner)
                                                     for _ in range(args.samples)))
    r = summary(per_round)
    arena_gb = n * 4 / 1e9
    a, b = r["a_sam"]["ms"], r["b_asam"]["ms"]
    print(json.dumps({
        "part": "kernels", "arena_floats": n, "chunks": (n + 4095) // 4096, **r,
        "gbps_by_arrays_moved": {"a": round(7 * arena_gb / a * 1e3, 1),
                                 "b": round(8 * arena_gb / b * 1e3, 1)},
        "sam_over_torch_device_scalar": round(a / r["c_torch_device_scalar"]["ms"], 4),
        "sam_over_torch_alpha": round(a / r["d_torch_alpha_host_scalar"]["ms"], 4),
        "out3": [float(x) for x in out3.tolist()]}), flush=True)


def plain_step_ms(args):
    """median ms of this tree's plain Config A step over `step_samples` windows (one round)"""
    m = model()
    batch = [t.cuda() for t in O.synthetic_batch(args.batch, seed=1)[:4]]
    tr = Trainer(m, CONFIG_A)
    fn = lambda: tr.train_step(*batch)
    warm({"plain": fn}, args.warmup)
    ms = statistics.median(event_ms(fn, args.steps) for _ in range(args.step_samples))
    tr.losses()
    return ms


def parent_round(args):
    """one round of the parent commit's plain step, in a process of its own"""
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", args.parent, "--child",
           "--batch", str(args.batch), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--step-samples", str(args.step_samples)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])["ms"]


def steps(args):
    batch = [t.cuda() for t in O.synthetic_batch(args.batch, seed=1)[:4]]
    cfgs = {"plain": CONFIG_A,
            "sam": TrainConfig(**{**CONFIG_A.__dict__, "sam_rho": 0.05}),
            "sam_every_2": TrainConfig(**{**CONFIG_A.__dict__, "sam_rho": 0.05, "sam_every": 2})}
    trs = {name: Trainer(model(), cfg) for name, cfg in cfgs.items()}
    cands = {name: (lambda tr=tr: tr.train_step(*batch)) for name, tr in trs.items()}
    warm(cands, args.warmup)
    per_round = {name: [] for name in cands}
    if args.parent:
        per_round["parent_plain"] = []
    for _ in range(args.rounds):
        if args.parent:
            per_round["parent_plain"].append(parent_round(args))
        for name, fn in cands.items():
            per_round[name].append(statistics.median(event_ms(fn, args.steps)
                                                     for _ in range(args.step_samples)))
    for tr in trs.values():
        tr.losses()                               # surfaces a bad status / non-finite loss
    r = summary(per_round)
    base = r["plain"]["ms"]
    out = {"part": "train_step", "batch": args.batch, "config": "A", **r,
           "steps_per_s": {k: round(1e3 / v["ms"], 2) for k, v in r.items()},
           "sam_over_plain": round(r["sam"]["ms"] / base, 4),
           "sam_minus_twice_plain_ms": round(r["sam"]["ms"] - 2 * base, 5),
           "sam_every_2_over_plain": round(r["sam_every_2"]["ms"] / base, 4),
           "sam_steps": {k: tr.sam_steps for k, tr in trs.items()},
           "largest_spread_ms": round(max(v["max"] - v["min"] for v in r.values()), 5)}
    if args.parent:
        out["plain_minus_parent_plain_ms"] = round(base - r["parent_plain"]["ms"], 5)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--samples", type=int, default=20, help="event windows per round (kernels)")
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per event window")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=30, help="train steps per event window")
    ap.add_argument("--step-samples", type=int, default=3, help="event windows per round (steps)")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--parent", default=None, help="built checkout of the parent commit")
    ap.add_argument("--tree", default=None, help="measure the package of this checkout instead")
    ap.add_argument("--child", action="store_true", help="one round of the plain step, one JSON line")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sam_bench.py measures on the device; there is no CPU path"
    if args.child:
        print(json.dumps({"ms": plain_step_ms(args), "tree": TREE}), flush=True)
        return
    assert args.rounds >= 3, "min / median / max need at least three rounds"
    kernels(args)
    if not args.no_steps:
        steps(args)


if __name__ == "__main__":
    main()
