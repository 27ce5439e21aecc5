#!/usr/bin/env python3
"""What the k nearest rows of a pool cost for MANY queries: NeighbourIndex.join's kernels
(cilrs_knn_join, csrc/knn_join.hip, plus cilrs_knn for the queries it cannot certify) against
  (i)  NeighbourIndex.query's path (cilrs_knn, one sweep of the pool per eight queries) on the same
       index and queries, and
  (ii) torch as a user would write it: the GEMM form xx - 2 Y X^T + yy in chunks of 4,096 queries with
       the distance block materialised, then topk.
Pool: N = 176,256 rows (the reference's training-set size) of F = 512 synthetic post-ReLU features
(relu of a Gaussian).  Q = 8 .. 16,384 fresh queries, and the whole pool against itself
(NeighbourIndex.graph, the leave-one-out self-join) where --graph asks for it; K = 1, 8, 16.

Protocol (tools/knn_bench.py): the candidates alternate in one process over the rounds; host
wall-clock around a call that ends in one synchronise; per candidate the median of each round's
calls, over the rounds the median of those and their max - min.  `join_beats_query`: ahead by more
than the larger spread.  `TFLOPs_entry` is 2 N Q F over the whole join call (norms, screen, merge,
re-score and fallback included), a lower bound of the screen launch's own rate; the launch itself is
read from a kernel trace of this tool (--trace-shape runs one call and nothing else).
--red-light: every row repeated 50 times under 1e-3 noise (a car waiting at a red light): more
near-ties than the screen keeps candidates, so most queries fall back.

One child process per K under a time limit; the parent stops at the first child that fails.  One
JSON line per configuration."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TFLOPS = 157.3


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
    return {name: dict(ms=round(statistics.median(v), 3), spread_ms=round(max(v) - min(v), 3),
                       rounds_ms=[round(x, 3) for x in v]) for name, v in per_round.items()}


def pool(args, torch):
    torch.manual_seed(0)
    N, F = args.rows, args.feat
    if not args.red_light:
        return torch.relu(torch.randn(N, F, device="cuda"))
    base = torch.relu(torch.randn(-(-N // 50), F, device="cuda"))
    X = base.repeat_interleave(50, dim=0)[:N].contiguous()
    return X + 1e-3 * torch.randn(N, F, device="cuda")


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd"))
    import torch
    from cilrs_mi355.neighbours import NeighbourIndex
    N, F, K = args.rows, args.feat, args.k
    X = pool(args, torch)
    index = NeighbourIndex(X)
    xx = (X * X).sum(1)
    tag = "red-light rows " if args.red_light else ""

    if args.trace_shape:
        Y = torch.relu(torch.randn(args.trace_shape, F, device="cuda"))
        for _ in range(2):
            index._join_rows(Y, K, None)
            torch.cuda.synchronize()
        return 0

    for Q in args.queries:
        Y = X[:Q] + 0.5 * torch.relu(torch.randn(Q, F, device="cuda")) if args.red_light else \
            torch.relu(torch.randn(Q, F, device="cuda"))
        got = {}

        def join():
            got["join"] = index._join_rows(Y, K, None)
            torch.cuda.synchronize()

        def query():
            got["query"] = index._query_rows(Y, K, None)
            torch.cuda.synchronize()

        @torch.no_grad()
        def gemm():
            out = []
            for q0 in range(0, Q, 4096):
                y = Y[q0:q0 + 4096]
                d = xx[None, :] - 2.0 * (y @ X.T) + (y * y).sum(1)[:, None]
                out.append(d.topk(K, dim=1, largest=False).indices)
            got["gemm"] = torch.cat(out)
            torch.cuda.synchronize()

        calls = 1 if Q >= 16384 else 3 if Q >= 1024 else 10
        r = measure({"join": join, "i_query": query, "ii_torch_gemm_topk": gemm}, calls, args.rounds, 1)
        ji, jd, flagged = got["join"]
        qi, qd = got["query"]
        spread = max(r["join"]["spread_ms"], r["i_query"]["spread_ms"])
        j = r["join"]["ms"]
        print(json.dumps({
            "config": f"{tag}N={N} F={F} Q={Q} K={K}", **r,
            "uncertified": f"{flagged}/{Q}",
            "TFLOPs_entry": round(2.0 * N * Q * F / (j * 1e-3) / 1e12, 2),
            "share_of_fp32_matrix_peak": round(2.0 * N * Q * F / (j * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
            "query_over_join": round(r["i_query"]["ms"] / j, 2),
            "torch_over_join": round(r["ii_torch_gemm_topk"]["ms"] / j, 2),
            "larger_spread_ms": spread,
            "join_beats_query": bool(r["i_query"]["ms"] - j > spread),
            "bits_equal_to_query": bool(torch.equal(ji, qi) and torch.equal(jd.view(torch.int32), qd.view(torch.int32))),
            "indices_equal_to_torch": f"{int((got['gemm'] == ji).sum())}/{Q * K}"}), flush=True)

    if args.graph:
        got = {}

        def graph():
            got["graph"] = index.graph(K)
            torch.cuda.synchronize()

        def loo_query():
            rows = torch.arange(N, device="cuda")
            out = [index._query_rows(X[q0:q0 + 65536], K, rows[q0:q0 + 65536]) for q0 in range(0, N, 65536)]
            got["query"] = (torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out]))
            torch.cuda.synchronize()

        cands = {"graph": graph}
        if args.graph_baseline:
            cands["i_query"] = loo_query
        r = measure(cands, 1, args.rounds, 1)
        g = r["graph"]["ms"]
        line = {"config": f"{tag}graph (self-join, leave-one-out) N=Q={N} F={F} K={K}", **r,
                "uncertified": f"{index.last_join['uncertified']}/{N}",
                "TFLOPs_entry": round(2.0 * N * N * F / (g * 1e-3) / 1e12, 2),
                "share_of_fp32_matrix_peak": round(2.0 * N * N * F / (g * 1e-3) / 1e12 / PEAK_TFLOPS, 3)}
        if args.graph_baseline:
            spread = max(v["spread_ms"] for v in r.values())
            line.update(query_over_graph=round(r["i_query"]["ms"] / g, 2), larger_spread_ms=spread,
                        graph_beats_query=bool(r["i_query"]["ms"] - g > spread),
                        bits_equal_to_query=bool(torch.equal(got["graph"][0], got["query"][0]) and
                                                 torch.equal(got["graph"][1].view(torch.int32),
                                                             got["query"][1].view(torch.int32))))
        print(json.dumps(line), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=176256)
    ap.add_argument("--feat", type=int, default=512)
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 8, 16])
    ap.add_argument("--queries", type=int, nargs="*", default=[8, 16, 32, 64, 128, 256, 1024, 16384])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--graph", action="store_true", help="also the self-join of the whole pool")
    ap.add_argument("--graph-baseline", action="store_true", help="... and the query path for it (slow)")
    ap.add_argument("--red-light", action="store_true", help="every row repeated 50 times under 1e-3 noise")
    ap.add_argument("--limit", type=int, default=400, help="seconds per K")
    ap.add_argument("--k", type=int, default=0, help="(child) run this one K in-process")
    ap.add_argument("--trace-shape", type=int, default=0,
                    help="(child) two join calls of this many queries and nothing else, for a kernel trace")
    args = ap.parse_args()
    if args.k:
        return child(args)
    common = ["--rows", str(args.rows), "--feat", str(args.feat), "--rounds", str(args.rounds), "--queries"] + \
        [str(q) for q in args.queries]
    for flag in ("graph", "graph_baseline", "red_light"):
        if getattr(args, flag):
            common.append("--" + flag.replace("_", "-"))
    for k in args.ks:
        cmd = [sys.executable, os.path.abspath(__file__), "--k", str(k)] + common
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
