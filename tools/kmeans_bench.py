#!/usr/bin/env python3
"""What one Lloyd iteration costs on the device (cilrs_kmeans_assign / _update / _lloyd,
csrc/kmeans.hip) against the torch realisation a user could write without it.

Pool: N = 176,256 rows (the reference's training-set size) of F = 512 synthetic post-ReLU features
(relu of a Gaussian), K = 16, 64 and 256 centres seeded from evenly spaced rows.
  (a) cilrs_kmeans_lloyd with iters = 1 minus its closing assignment: assign + update, the six
      launches of an iteration; timed as lloyd(iters = 1) and as assign and update on their own.
  (b) torch: torch.cdist(X, C).argmin(1), zeros(K, F).index_add_(0, label, X), bincount, a division
      (the N x K distances are materialised and the sums use floating-point atomics: not
      reproducible from run to run).
The two alternate in one process over the rounds.  The calls are a few hundred microseconds, so a
sample is host wall-clock around `reps` calls enqueued back to back and one synchronise, divided by
reps; per candidate the median of each round's samples, over the rounds the median of those and
their max - min.  Reported with the bandwidth the assignment reaches over N F 4 bytes and its share
of the fp32 vector issue rate in subtract + fma: 2 N K F lane operations against 256 CUs x 4 SIMDs x
32 lanes x 2.4 GHz = 78.6e12 per second (the 157.3 TFLOP/s fp32 vector peak counts an fma as two).

Every K runs in a child process of its own under a time limit; the parent stops at the first child
that fails.  One JSON line per K."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
ASSIGN_ESTIMATE_US = 150.0       # K = 64: the subtract + fma at the vector issue rate


def measure(cands, reps, samples, rounds, warmup, sync):
    for fn in cands.values():
        for _ in range(warmup):
            fn()
        sync()
    per_round = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            ts = []
            for _ in range(samples):
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                sync()
                ts.append((time.perf_counter() - t0) / reps)
            per_round[name].append(statistics.median(ts) * 1e6)
    return per_round


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd"))
    import torch
    from cilrs_mi355 import _lib as L
    N, F, K = args.rows, args.feat, args.k
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    X = torch.relu(torch.randn(N, F, device=dev))
    C0 = X[torch.arange(K, device=dev) * (N // K)].contiguous()
    lib = L.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = lib.cilrs_kmeans_scratch_bytes(N, F, K)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    Cd = C0.clone()
    label = torch.full((N,), -1, dtype=torch.int32, device=dev)
    dist = torch.empty(N, dtype=torch.float32, device=dev)
    counts = torch.empty(K, dtype=torch.int64, device=dev)
    inertia = torch.empty(2, dtype=torch.float64, device=dev)
    changed = torch.empty(2, dtype=torch.int64, device=dev)

    def assign():
        L.check(lib.cilrs_kmeans_assign(L.ptr(X), F, N, F, L.ptr(Cd), F, K, L.ptr(label), L.ptr(dist),
                                        L.ptr(counts), L.ptr(inertia), L.ptr(changed), L.ptr(scratch), nbytes,
                                        stream()))

    def update():
        L.check(lib.cilrs_kmeans_update(L.ptr(X), F, N, F, L.ptr(label), L.ptr(Cd), F, K, L.ptr(counts),
                                        L.ptr(scratch), nbytes, stream()))

    def lloyd1():
        L.check(lib.cilrs_kmeans_lloyd(L.ptr(X), F, N, F, L.ptr(Cd), F, K, 1, L.ptr(label), L.ptr(dist),
                                       L.ptr(counts), L.ptr(inertia), L.ptr(changed), L.ptr(scratch), nbytes,
                                       stream()))

    Ct = C0.clone()

    @torch.no_grad()
    def torch_iter():
        lab = torch.cdist(X, Ct).argmin(1)
        S = torch.zeros(K, F, device=dev).index_add_(0, lab, X)
        n = torch.bincount(lab, minlength=K)
        Ct.copy_(torch.where(n[:, None] > 0, S / n.clamp(min=1)[:, None], Ct))

    @torch.no_grad()
    def torch_assign():
        return torch.cdist(X, Ct).argmin(1)

    assign()                                                 # labels for update() on its own
    torch.cuda.synchronize()
    r = measure({"a_assign": assign, "a_update": update, "a_lloyd_1": lloyd1, "b_torch_iteration": torch_iter,
                 "b_torch_cdist_argmin": torch_assign}, args.reps, args.samples, args.rounds, 2,
                torch.cuda.synchronize)
    out = {"config": f"N={N} F={F} K={K}", "pool_MB": round(N * F * 4 / 1e6, 1), "scratch_MB": round(nbytes / 1e6, 2)}
    med, spread = {}, {}
    for name, v in r.items():
        med[name], spread[name] = statistics.median(v), max(v) - min(v)
        out[name] = dict(us=round(med[name], 1), spread_us=round(spread[name], 1), rounds_us=[round(x, 1) for x in v])
    # an iteration = lloyd(iters = 1) less its closing assignment; also assign + update as timed alone
    it = med["a_lloyd_1"] - med["a_assign"]
    it_spread = spread["a_lloyd_1"] + spread["a_assign"]
    out["a_iteration_us"] = round(it, 1)
    out["a_assign_plus_update_us"] = round(med["a_assign"] + med["a_update"], 1)
    gain = med["b_torch_iteration"] - it
    big = max(it_spread, spread["b_torch_iteration"])
    out["torch_minus_kmeans_us"] = round(gain, 1)
    out["largest_spread_us"] = round(big, 1)
    out["kmeans_beats_torch"] = bool(gain > big)
    out["assign_TB_per_s"] = round(N * F * 4 / (med["a_assign"] * 1e-6) / 1e12, 3)
    out["update_TB_per_s"] = round(N * F * 4 / (med["a_update"] * 1e-6) / 1e12, 3)
    out["assign_share_of_vector_issue_rate"] = round(2.0 * N * K * F / LANE_OPS_PER_S / (med["a_assign"] * 1e-6), 3)
    if K == 64:
        out["assign_estimate_us"] = ASSIGN_ESTIMATE_US
    # do the two agree?  labels of one assignment on the same centres
    Cd.copy_(C0)
    Ct.copy_(C0)
    assign()
    lab = torch_assign()
    torch.cuda.synchronize()
    out["labels_equal_to_torch"] = int((lab == label).sum())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=176256)
    ap.add_argument("--feat", type=int, default=512)
    ap.add_argument("--ks", type=int, nargs="*", default=[16, 64, 256])
    ap.add_argument("--reps", type=int, default=10, help="calls per sample, one synchronise at the end")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per K")
    ap.add_argument("--k", type=int, default=0, help="(child) run this one K in-process")
    args = ap.parse_args()
    if args.k:
        return child(args)
    for k in args.ks:
        cmd = [sys.executable, os.path.abspath(__file__), "--k", str(k), "--rows", str(args.rows), "--feat",
               str(args.feat), "--reps", str(args.reps), "--samples", str(args.samples), "--rounds",
               str(args.rounds)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"K={k}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
