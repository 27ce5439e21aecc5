#!/usr/bin/env python3
"""What a greedy k-center pick costs on the device (cilrs_kcenter_greedy, csrc/kcenter.hip) against
the torch loop a user could write without it.

Pool: N = 176,256 rows (the reference's training-set size) of F = 512 and 2048 synthetic post-ReLU
features (relu of a Gaussian), K = 256 picks from a +inf start.
  (a) cilrs_kcenter_greedy: K + 1 launches, no temporaries.
  (b) torch: per pick argmax(mind), ((X - X[i]) ** 2).sum(1), torch.minimum -- the index stays on the
      device, nothing synchronises inside the loop.
The two alternate in one process over the rounds; host wall-clock around a call that ends in one
synchronise; per candidate the median of each round's calls, over the rounds the median of those and
their max - min.  Reported per pick, with the bandwidth that implies over N F 4 bytes; the floor to
compare with is one sweep of the pool at the 6.3 TB/s a float4 copy reaches on this part.  Also
timed: cilrs_kcenter_cover of eight centres and the one-off whitening GEMM of the pool.

Every configuration runs in a child process of its own under a time limit; the parent stops at the
first child that fails.  One JSON line per configuration."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_TBS = 6.3


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
    return per_round


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd"))
    import torch
    from cilrs_mi355 import _lib as L
    N, F, K = args.rows, args.feat, args.picks
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    X = torch.relu(torch.randn(N, F, device=dev))
    lib = L.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = lib.cilrs_kcenter_scratch_bytes(N)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mind = torch.empty(N, dtype=torch.float32, device=dev)
    sel = torch.empty(K, dtype=torch.int64, device=dev)
    radius = torch.empty(K, dtype=torch.float32, device=dev)
    sel_t, radius_t = torch.empty_like(sel), torch.empty_like(radius)

    def hip():
        mind.fill_(float("inf"))
        L.check(lib.cilrs_kcenter_greedy(L.ptr(X), F, N, F, L.ptr(mind), K, L.ptr(sel), L.ptr(radius),
                                         L.ptr(scratch), nbytes, stream()))
        torch.cuda.synchronize()

    @torch.no_grad()
    def loop():
        m = torch.full((N,), float("inf"), device=dev)
        for t in range(K):
            i = torch.argmax(m)
            sel_t[t] = i
            radius_t[t] = m[i]
            m = torch.minimum(m, ((X - X[i]) ** 2).sum(1))
        torch.cuda.synchronize()

    r = measure({"a_kcenter_greedy": hip, "b_torch_loop": loop}, args.calls, args.rounds, 1)
    out = {"config": f"N={N} F={F} K={K}", "pool_MB": round(N * F * 4 / 1e6, 1),
           "sweep_floor_us": round(N * F * 4 / (SWEEP_TBS * 1e12) * 1e6, 1)}
    spreads = []
    for name, v in r.items():
        us = [x * 1e3 / K for x in v]
        med = statistics.median(us)
        spreads.append(max(us) - min(us))
        out[name] = dict(us_per_pick=round(med, 2), spread_us=round(spreads[-1], 2),
                         TB_per_s=round(N * F * 4 / (med * 1e-6) / 1e12, 3),
                         rounds_us=[round(x, 2) for x in us])
    gain = out["b_torch_loop"]["us_per_pick"] - out["a_kcenter_greedy"]["us_per_pick"]
    out["torch_minus_kcenter_us"] = round(gain, 2)
    out["largest_spread_us"] = round(max(spreads), 2)
    out["kcenter_beats_torch"] = bool(gain > max(spreads))
    out["share_of_sweep_bandwidth"] = round(out["a_kcenter_greedy"]["TB_per_s"] / SWEEP_TBS, 3)
    # the two sequences: the same picks until the first near-tie the summation orders split
    same = (sel == sel_t).cpu().numpy()
    out["picks_equal_to_torch"] = int(same.sum())
    out["first_pick_that_differs"] = int(same.argmin()) if not same.all() else None

    centres = X[torch.arange(8, device=dev) * (N // 8)].contiguous()

    def cover():
        mind.fill_(float("inf"))
        L.check(lib.cilrs_kcenter_cover(L.ptr(X), F, N, F, L.ptr(centres), F, 8, L.ptr(mind), stream()))
        torch.cuda.synchronize()

    W = torch.tril(torch.randn(F, F, device=dev)) / F ** 0.5
    origin = X[:64].mean(dim=0)

    @torch.no_grad()
    def whiten():
        z = (X - origin) @ W.T
        torch.cuda.synchronize()
        return z

    r = measure({"cover_8_centres": cover, "whitening_gemm": whiten}, 5, args.rounds, 2)
    for name, v in r.items():
        out[name] = dict(ms=round(statistics.median(v), 4), spread=round(max(v) - min(v), 4))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=176256)
    ap.add_argument("--feats", type=int, nargs="*", default=[512, 2048])
    ap.add_argument("--picks", type=int, default=256)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--feat", type=int, default=0, help="(child) run this one width in-process")
    args = ap.parse_args()
    if args.feat:
        return child(args)
    for feat in args.feats:
        cmd = [sys.executable, os.path.abspath(__file__), "--feat", str(feat), "--rows", str(args.rows),
               "--picks", str(args.picks), "--calls", str(args.calls), "--rounds", str(args.rounds)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"F={feat}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
