"""Times of the input-gradient path at the benchmark geometry (default B = 128, 200x88):
  * the stem data-gradient kernel (cilrs_stem_conv_dgrad) beside the stem forward kernel
    (cilrs_stem_conv_fwd) of the same geometry, launched back to back in one process;
  * an eval-mode saliency pass: model.eval(), parameters frozen, image.requires_grad_(),
    forward (frozen BatchNorm) + torch.autograd.grad(controls.sum(), image), against the plain
    eval forward under torch.no_grad() -- the backward is the data-gradient-only one
    (cilrs_net_backward_data); --profile adds its per-label device times (one serialised pass);
  * one frame through Predictor.saliency (upload, frozen forward, data-only backward, heat map,
    read-back) beside Predictor.predict_batch of the same frame, as host wall-clock per call.
Per item: (median, min, max) of --rounds rounds of --iters launches each, timed with device events
after --warmup launches.  Prints one JSON line.
--attribution runs, instead of all that, Predictor.attribution (SmoothGrad and integrated
gradients, one frame, --samples samples) per candidate chunk against a Python loop of as many
Predictor.saliency calls -- see attribution_bench.

    python tools/input_grad_bench.py [--batch 128] [--height 88] [--width 200] [--profile]
    python tools/input_grad_bench.py --attribution [--samples 32]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed_ms(fn, iters, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out), min(out), max(out)


def wall_ms(fn, iters, rounds, warmup):
    """Synchronous calls (they end with their own stream synchronisation): host time per call."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def attribution_bench(samples, rounds, reps):
    """One 88x200 frame, `samples` samples: Predictor.attribution per candidate `chunk` beside the
    documented workaround it replaces, a Python loop of `samples` Predictor.saliency calls.  Per
    candidate the two are alternated for `rounds` rounds in this one process; a round times the
    loop once and the mean of `reps` attribution calls (host wall-clock: both end in their own
    stream synchronisation).  The batched call counts as faster only if it beats the loop by more
    than the loop's own max - min over the rounds."""
    import cilrs_oracle as O
    from cilrs_mi355 import CILRS
    from cilrs_mi355.predict import Predictor
    m = CILRS(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
    m = m.cuda().eval().requires_grad_(False)
    pr = Predictor(m)
    frame = O.synthetic_batch(1, seed=4)[4]

    def loop():
        for _ in range(samples):
            pr.saliency(frame, [30.0], [1])

    def once(fn, n=1):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n

    res = {"samples": samples, "rounds": rounds, "reps": reps, "default_chunk": Predictor.ATTRIBUTION_CHUNK,
           "chunks": {}}
    for chunk in sorted({min(samples, c) for c in (8, 16, 32)}):
        def smooth():
            pr.attribution(frame, [30.0], [1], method="smoothgrad", samples=samples, chunk=chunk)

        def integrated():
            pr.attribution(frame, [30.0], [1], method="integrated", samples=samples, chunk=chunk)
        for fn in (loop, smooth, integrated, loop, smooth, integrated):     # plans, code objects
            fn()
        row = {"saliency_loop_ms": [], "smoothgrad_ms": [], "integrated_ms": []}
        for _ in range(rounds):
            row["saliency_loop_ms"].append(once(loop))
            row["smoothgrad_ms"].append(once(smooth, reps))
            row["integrated_ms"].append(once(integrated, reps))
        lp = row["saliency_loop_ms"]
        spread = max(lp) - min(lp)
        row["loop_spread_ms"] = spread
        for k in ("smoothgrad_ms", "integrated_ms"):
            row[k.replace("_ms", "_faster_beyond_spread")] = \
                statistics.median(lp) - statistics.median(row[k]) > spread
        res["chunks"][str(chunk)] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attribution", action="store_true",
                    help="only: Predictor.attribution (one frame, --samples samples, chunk 8 / 16 / "
                         "32) against a loop of Predictor.saliency calls, alternated, three rounds")
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--height", type=int, default=88)
    ap.add_argument("--width", type=int, default=200)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true",
                    help="per-label device times of one saliency pass (serialised launches)")
    a = ap.parse_args()
    if a.attribution:
        print(json.dumps(attribution_bench(a.samples, 3, 5)))
        return
    import cilrs_oracle as O
    from cilrs_mi355 import CILRS, _lib as L
    lib = L.lib()
    B, H, W = a.batch, a.height, a.width
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(0)
    x4 = torch.randn(B, H, W, 4, device="cuda", generator=g)
    x4[..., 3] = 0
    w = torch.randn(64, 7, 7, 3, device="cuda", generator=g) * 0.1
    y = torch.empty(B, Ho, Wo, 64, device="cuda")
    dy = torch.randn(B, Ho, Wo, 64, device="cuda", generator=g)
    dx = torch.empty(B, 3, H, W, device="cuda")
    rows = C.c_int()

    def fwd():
        L.check(lib.cilrs_stem_conv_fwd(L.ptr(x4), L.ptr(w), L.ptr(y), None, B, H, W, C.byref(rows), st))

    def dgrad():
        L.check(lib.cilrs_stem_conv_dgrad(L.ptr(dy), L.ptr(w), L.ptr(dx), *dx.stride(), B, H, W, st))

    res = {"batch": B, "height": H, "width": W}
    try:                      # (the register-resident stem forward serves widths up to 445)
        res["stem_fwd_ms"] = timed_ms(fwd, a.iters, a.rounds, a.warmup)
    except RuntimeError as e:
        res["stem_fwd_ms"] = str(e)
    res["stem_dgrad_ms"] = timed_ms(dgrad, a.iters, a.rounds, a.warmup)
    useful = 2.0 * B * Ho * Wo * 64 * 147
    res["stem_dgrad_useful_tflops"] = useful / (res["stem_dgrad_ms"][0] * 1e-3) / 1e12
    if isinstance(res["stem_fwd_ms"], tuple):
        res["dgrad_over_fwd"] = res["stem_dgrad_ms"][0] / res["stem_fwd_ms"][0]

    m = CILRS(4, 0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 0))
    m = m.cuda().eval().requires_grad_(False)
    imgs, spds, cmds = (t.cuda() for t in O.synthetic_batch(B, seed=3, h=H, w=W)[:3])

    def infer():
        with torch.no_grad():
            m(imgs, spds, cmds)

    def saliency():
        x = imgs.detach().requires_grad_()
        c, _ = m(x, spds, cmds)
        torch.autograd.grad(c.sum(), x)

    res["eval_forward_ms"] = timed_ms(infer, max(1, a.iters // 4), a.rounds, a.warmup)
    res["saliency_fwd_bwd_ms"] = timed_ms(saliency, max(1, a.iters // 4), a.rounds, a.warmup)
    if a.profile:
        pl = m.engine().plan(B, H, W)
        pl.profile(True)
        try:
            pl.profile_reset()
            saliency()
            torch.cuda.synchronize()
            rows = pl.profile_table()
        finally:
            pl.profile(False)
        res["saliency_profile_ms"] = {k: [r["calls"], round(r["ms"], 4)] for k, r in sorted(rows.items())}

    # one frame: the control loop's tick beside its saliency map
    from cilrs_mi355.predict import Predictor
    pr = Predictor(m)
    frame = O.synthetic_batch(1, seed=4)[4]
    res["predict_batch_b1_ms"] = wall_ms(lambda: pr.predict_batch(frame, [30.0], [1]), a.iters,
                                         a.rounds, a.warmup)
    res["predictor_saliency_b1_ms"] = wall_ms(lambda: pr.saliency(frame, [30.0], [1]), a.iters,
                                              a.rounds, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
