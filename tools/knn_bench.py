#!/usr/bin/env python3
"""What the k nearest rows of a pool cost on the device (cilrs_knn, csrc/knn.hip) against the two
torch forms a user could write without it, and what Predictor.predict_neighbours adds to a tick.

Op level.  Pool: N = 176,256 rows (the reference's training-set size) of F = 512 and 2048 synthetic
post-ReLU features (relu of a Gaussian); Q = 1 and 8 queries; K = 8 and 64.
  (a) cilrs_knn: two launches per chunk of eight queries, no temporaries beyond the scratch.
  (b) torch: ((X - y) ** 2).sum(1).topk(K, largest=False) per query.
  (c) torch: (xx - 2 X @ Y.T + yy).topk(K, dim=0, largest=False) with the row norms xx precomputed.
The three alternate in one process over the rounds; host wall-clock around a call that ends in one
synchronise; per candidate the median of each round's calls, over the rounds the median of those and
their max - min.  The floor to compare with is one sweep of the pool at the 6.3 TB/s a float4 copy
reaches on this part (per chunk of eight queries).  Also timed: the one-off whitening of the pool
through cilrs_feature_whiten (NeighbourIndex.whiten, in chunks) against the torch GEMM.

Tick.  B = 1, 88x200 on the persistent predictor, one process: predict_batch, predict_neighbours
(k = 8) against a 176,256-row and a 16,384-row Mahalanobis index of synthetic rows, and
predict_novelty beside them.

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
            per_round[name].append(statistics.median(ts) * 1e6)
    return {name: dict(us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2),
                       rounds_us=[round(x, 2) for x in v]) for name, v in per_round.items()}


def child_op(args):
    sys.path.insert(0, os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd"))
    import torch
    from cilrs_mi355 import _lib as L
    from cilrs_mi355.neighbours import NeighbourIndex
    N, F = args.rows, args.feat
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    X = torch.relu(torch.randn(N, F, device=dev))
    xx = (X * X).sum(1)
    lib = L.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    floor = N * F * 4 / (SWEEP_TBS * 1e12) * 1e6
    for Q in (1, 8):
        Y = torch.relu(torch.randn(Q, F, device=dev))
        for K in (8, 64):
            nbytes = lib.cilrs_knn_scratch_bytes(N, Q, K)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            idx = torch.empty(Q, K, dtype=torch.int64, device=dev)
            dist = torch.empty(Q, K, dtype=torch.float32, device=dev)
            got = {}

            def hip():
                L.check(lib.cilrs_knn(L.ptr(X), F, N, F, L.ptr(Y), F, Q, None, K, L.ptr(idx), L.ptr(dist),
                                      L.ptr(scratch), nbytes, stream()))
                torch.cuda.synchronize()

            @torch.no_grad()
            def diff():
                got["b"] = [((X - Y[q]) ** 2).sum(1).topk(K, largest=False) for q in range(Q)]
                torch.cuda.synchronize()

            @torch.no_grad()
            def gemm():
                d = xx[:, None] - 2.0 * (X @ Y.T) + (Y * Y).sum(1)[None, :]
                got["c"] = d.topk(K, dim=0, largest=False)
                torch.cuda.synchronize()

            r = measure({"a_cilrs_knn": hip, "b_torch_diff_topk": diff, "c_torch_gemm_topk": gemm},
                        args.calls, args.rounds, 3)
            spread = max(v["spread_us"] for v in r.values())
            a = r["a_cilrs_knn"]["us"]
            same_b = sum(int((got["b"][q].indices == idx[q]).sum()) for q in range(Q))
            same_c = int((got["c"].indices.T == idx).sum())
            print(json.dumps({
                "config": f"N={N} F={F} Q={Q} K={K}", "sweep_floor_us": round(floor, 1), **r,
                "TB_per_s": round(N * F * 4 / (a * 1e-6) / 1e12, 3),
                "share_of_sweep_bandwidth": round(floor / a, 3),
                "b_minus_a_us": round(r["b_torch_diff_topk"]["us"] - a, 2),
                "c_minus_a_us": round(r["c_torch_gemm_topk"]["us"] - a, 2),
                "largest_spread_us": spread,
                "a_beats_b": bool(r["b_torch_diff_topk"]["us"] - a > spread),
                "a_beats_c": bool(r["c_torch_gemm_topk"]["us"] - a > spread),
                "indices_equal_to_b": f"{same_b}/{Q * K}", "indices_equal_to_c": f"{same_c}/{Q * K}"}),
                flush=True)
    # the one-off whitening of the pool
    W = torch.tril(torch.randn(F, F, device=dev)) / F ** 0.5
    origin = X[:64].mean(dim=0)
    index = NeighbourIndex(X[:8], "mahalanobis", origin, W)

    def whiten_hip():
        z = index.whiten(X)
        torch.cuda.synchronize()
        return z

    @torch.no_grad()
    def whiten_gemm():
        z = (X - origin) @ W.T
        torch.cuda.synchronize()
        return z

    r = measure({"cilrs_feature_whiten": whiten_hip, "torch_gemm": whiten_gemm}, 3, args.rounds, 1)
    print(json.dumps({"config": f"whitening of the pool N={N} F={F}",
                      **{k: dict(ms=round(v["us"] / 1e3, 3), spread_ms=round(v["spread_us"] / 1e3, 3))
                         for k, v in r.items()}}), flush=True)


def child_tick(args):
    for p in ("cilrs-autonomous-driving-carla_amd", "oracle"):
        sys.path.insert(0, os.path.join(ROOT, p))
    import torch
    import cilrs_oracle as O
    from cilrs_mi355 import CILRS
    from cilrs_mi355.neighbours import NeighbourIndex
    from cilrs_mi355.novelty import FeatureDensity
    from cilrs_mi355.predict import Predictor
    m = CILRS(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
    m = m.cuda().eval()
    fd = FeatureDensity(m)
    for i in range(3):
        img, spd, cmd, _t, _u8 = O.synthetic_batch(128, seed=10 + i)
        fd.update(img.cuda(), spd.cuda(), cmd.cuda())
    fd.finalize()
    torch.manual_seed(0)
    rows = torch.relu(torch.randn(args.rows, fd.F, device="cuda"))
    big = NeighbourIndex(rows, "mahalanobis", fd._origin().clone(), fd.W.clone(), commands=fd.NC,
                         whitened=False)
    core = NeighbourIndex(big.rows[:16384].clone(), "mahalanobis", big.origin, big.W, commands=fd.NC)
    pred = Predictor(m)
    u8 = O.synthetic_batch(1, seed=1)[4]
    kmh, cmd = [30.0], [2]
    cands = {
        "predict_batch": lambda: pred.predict_batch(u8, kmh, cmd),
        f"predict_neighbours_{len(big)}": lambda: pred.predict_neighbours(u8, kmh, cmd, big, k=8),
        f"predict_neighbours_{len(core)}": lambda: pred.predict_neighbours(u8, kmh, cmd, core, k=8),
        "predict_novelty": lambda: pred.predict_novelty(u8, kmh, cmd, fd),
    }
    r = measure(cands, args.tick_calls, args.rounds, 50)
    tick = r["predict_batch"]["us"]
    print(json.dumps({"config": f"tick B=1 88x200 resnet34 F={fd.F} "
                                f"{'persistent' if pred.persistent else 'per-layer'} k=8", **r,
                      "added_us": {k: round(v["us"] - tick, 2) for k, v in r.items() if k != "predict_batch"},
                      "largest_spread_us": max(v["spread_us"] for v in r.values())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=176256)
    ap.add_argument("--feats", type=int, nargs="*", default=[512, 2048])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--tick-calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--feat", type=int, default=0, help="(child) run this one width in-process")
    ap.add_argument("--tick", action="store_true", help="(child) run the tick in-process")
    args = ap.parse_args()
    if args.feat:
        return child_op(args)
    if args.tick:
        return child_tick(args)
    common = ["--rows", str(args.rows), "--calls", str(args.calls), "--rounds", str(args.rounds),
              "--tick-calls", str(args.tick_calls)]
    for extra in [["--feat", str(f)] for f in args.feats] + [["--tick"]]:
        cmd = [sys.executable, os.path.abspath(__file__)] + extra + common
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"{' '.join(extra)}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
