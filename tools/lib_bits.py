#!/usr/bin/env python3
"""Does another build of libcilrs_hip.so compute the same bits and issue the same launches?

    CILRS_LIB=/path/to/parent/libcilrs_hip.so python tools/lib_bits.py dump /tmp/bits_parent
    python tools/lib_bits.py dump /tmp/bits_this
    python tools/lib_bits.py compare /tmp/bits_parent /tmp/bits_this

`dump` runs every case below in a fresh child process (the library reads its switches and caches
its kernel attributes once per process), one at a time, each under its own time limit; it stops at
the first child that does not exit normally and starts nothing after it.  A case writes its
tensors to <dir>/<case>.pt and, for the profile cases, the profile table's rows (label, calls,
flops, bytes) to <dir>/<case>.rows.json.  `compare` wants every tensor torch.equal and every sorted
row list identical, prints one line per tensor / table and a verdict, and exits non-zero otherwise.

Both libraries are driven by this tree's Python package; inputs and weights are seeded here (no
oracle, no files).  What a refactor of csrc/net.hip that changes no kernel has to show: the
profiles/*_ab.log files.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd"))

H, W = 88, 200
TRAIN_CASES = ("fp32", "bf16", "resnet50", "ft2", "frozen_data_only")
CASES = (["case." + c for c in TRAIN_CASES] + ["case.fp32_b32", "trainer.fused0", "trainer.fused1"] +
         ["infer.%s.%s" % (p, m) for p in ("fp32", "f16", "bf16") for m in ("eager", "graph")] +
         ["infer.b1.persistent", "infer.b1.camera"] +
         ["profile." + c for c in ("fp32", "bf16", "resnet50", "frozen_data_only")])
CHILD_TIMEOUT_S = 240


def _batch(b, seed=61, h=H, w=W):
    import torch
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(b, 3, h, w, generator=g)
    spd = torch.rand(b, generator=g)
    cmd = torch.randint(0, 4, (b,), generator=g)
    tgt = torch.rand(b, 3, generator=g) * 2 - 1
    frames = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
    return [t.cuda() for t in (img, spd, cmd, tgt, frames)]


def _model(resnet50=False):
    """seeded weights, BatchNorm buffers away from their (0, 1) start"""
    import torch
    from cilrs_mi355 import CILRS, CILRSResNet50
    torch.manual_seed(5)
    m = (CILRSResNet50 if resnet50 else CILRS)(num_commands=4, dropout=0.0)
    g = torch.Generator().manual_seed(7)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return m.cuda()


def _graph_pass(kind, b, profile=False):
    """one forward and one backward over all six segments (profile: with the profile table on)"""
    import torch
    img, spd, cmd, tgt, _ = _batch(b)
    m = _model(kind == "resnet50")
    eng = m.engine()
    data_only = kind == "frozen_data_only"
    if kind == "bf16":
        eng.train_precision = "bf16"
    if profile:
        eng.plan(b, H, W).profile(True)
    if data_only:
        m.eval()
        ctl, ps, pl = eng.run_forward_frozen(img, spd, cmd)
    elif kind == "ft2":
        m.train()
        ctl, ps, pl = eng.run_forward_ft(img, spd, cmd, 2, 2, 0.0, 0)
    else:
        m.train()
        ctl, ps, pl = eng.run_forward(img, spd, cmd, True, 0.0, 0)
    assert pl is eng.plan(b, H, W)
    eng.run_backward(pl, tgt.contiguous(), spd.contiguous(), data_only=data_only)
    out = {"controls": ctl, "pred_speed": ps, "params": eng.params, "bn": eng.bn}
    if data_only:
        out["dimage"] = torch.empty(b, 3, H, W, device=eng.device)
        out["dspeed"] = torch.empty(b, device=eng.device)
        eng.run_input_grads(pl, out["dimage"], out["dspeed"])
    else:
        out["grads"] = eng.grads
    torch.cuda.synchronize()
    pl.check_status()
    return out, pl


def _trainer(b, steps, fused, precision="fp32", resnet50=False, profile=False):
    import torch
    from cilrs_mi355 import CONFIG_A, Trainer
    img, spd, cmd, tgt, _ = _batch(b)
    m = _model(resnet50)
    tr = Trainer(m, CONFIG_A, precision=precision)
    tr.fuse_optimizer = bool(fused)
    pl = tr.eng.plan(b, H, W)
    if profile:
        pl.profile(True)
    losses = []
    for _ in range(steps):
        tr.train_step(img, spd, cmd, tgt)
        losses.append(tr.losses()["total"])
    out = {"params": tr.eng.params, "grads": tr.eng.grads, "bn": tr.eng.bn, "exp_avg": tr.exp_avg,
           "exp_avg_sq": tr.exp_avg_sq, "losses": torch.tensor(losses)}
    if not profile:
        m.eval()
        with torch.no_grad():
            out["controls"], out["pred_speed"] = m(img, spd, cmd)
    torch.cuda.synchronize()
    return out, pl


def _infer(precision, mode, b):
    import torch
    _, spd, cmd, _, frames = _batch(b)
    m = _model().eval()
    eng = m.engine()
    half = {"fp32": False, "f16": True, "bf16": "bf16"}[precision]
    with torch.cuda.stream(torch.cuda.Stream()):      # (a captured graph needs a stream of its own)
        if mode == "camera":
            raw = torch.randint(0, 256, (b, 300, 400, 4), dtype=torch.uint8,
                                generator=torch.Generator().manual_seed(9)).cuda()
            ctl, ps = eng.run_forward_camera(raw, spd, cmd, H, W)
        else:
            out = (torch.empty(b, 3, device=eng.device), torch.empty(b, device=eng.device))
            for _ in range(3 if mode == "graph" else 1):       # capture, then two replays
                ctl, ps = eng.run_forward_u8(frames, spd, cmd, out=out, graph=mode == "graph", half=half,
                                             persistent=mode == "persistent")
        torch.cuda.synchronize()
    eng.check_status()
    return {"controls": ctl, "pred_speed": ps}


def run_case(name, outdir):
    import torch
    group, _, rest = name.partition(".")
    rows = None
    if group == "case" and rest == "fp32_b32":
        out, pl = _trainer(32, 1, fused=False)
        assert pl.wino_convs() > 0, "the batch-32 plan has no Winograd layer"
    elif group == "case":
        out, _ = _graph_pass(rest, 4)
    elif group == "trainer":
        out, _ = _trainer(16, 3, fused=rest == "fused1")
    elif group == "infer":
        precision, mode = rest.split(".")
        out = _infer("fp32" if precision == "b1" else precision, mode, 1 if precision == "b1" else 4)
    else:
        assert group == "profile", name
        if rest == "frozen_data_only":
            _, pl = _graph_pass(rest, 4, profile=True)
        else:
            _, pl = _trainer(4, 1, fused=False, precision="bf16" if rest == "bf16" else "fp32",
                             resnet50=rest == "resnet50", profile=True)
        out = {}
        rows = sorted([k, v["calls"], v["flops"], v["bytes"]] for k, v in pl.profile_table().items())
    if out:
        torch.save({k: v.detach().cpu().clone() for k, v in out.items()}, os.path.join(outdir, name + ".pt"))
    if rows is not None:
        with open(os.path.join(outdir, name + ".rows.json"), "w") as f:
            json.dump(rows, f)
    print("DONE", name, flush=True)


def dump(outdir, only):
    os.makedirs(outdir, exist_ok=True)
    for name in only or CASES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "case", name, outdir],
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print("STOP %s: no exit within %d s" % (name, CHILD_TIMEOUT_S), flush=True)
            return 1
        tail = (r.stdout + r.stderr)[-1500:]
        if r.returncode != 0 or "DONE " + name not in r.stdout:
            print("STOP %s: exit %d\n%s" % (name, r.returncode, tail), flush=True)
            return 1
        print("ok   %s" % name, flush=True)
    return 0


def compare(dir_a, dir_b):
    import torch
    bad = n = nbytes = 0
    files = sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b)))
    for fn in files:
        pa, pb = os.path.join(dir_a, fn), os.path.join(dir_b, fn)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print("MISSING   %s" % fn)
            bad += 1
        elif fn.endswith(".rows.json"):
            ra, rb = json.load(open(pa)), json.load(open(pb))
            same = ra == rb
            bad += not same
            print("%-9s %-44s %d rows, %d calls" % ("SAME ROWS" if same else "DIFFERENT", fn[:-10], len(ra),
                                                    sum(r[1] for r in ra)))
        elif fn.endswith(".pt"):
            ta, tb = torch.load(pa), torch.load(pb)
            for k in sorted(set(ta) | set(tb)):
                same = k in ta and k in tb and torch.equal(ta[k], tb[k])
                bad += not same
                n += 1
                t = ta.get(k, tb.get(k))
                nbytes += t.numel() * t.element_size()
                print("%-9s %-44s %s absmax %g finite %s" % (
                    "EQUAL" if same else "DIFFERENT", fn[:-3] + "." + k, tuple(t.shape),
                    float(t.double().abs().max()), bool(torch.isfinite(t.double()).all())))
    print("bit equality: %d tensors, %d bytes" % (n, nbytes))
    print("VERDICT: %s" % ("ALL EQUAL, ROWS IDENTICAL" if bad == 0 else "%d DIFFERENCES" % bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("outdir")
    d.add_argument("--only", nargs="*", choices=CASES)
    c = sub.add_parser("case")
    c.add_argument("name", choices=CASES)
    c.add_argument("outdir")
    k = sub.add_parser("compare")
    k.add_argument("dir_a")
    k.add_argument("dir_b")
    args = ap.parse_args()
    if args.cmd == "dump":
        sys.exit(dump(args.outdir, args.only))
    if args.cmd == "case":
        run_case(args.name, args.outdir)
    else:
        sys.exit(compare(args.dir_a, args.dir_b))


if __name__ == "__main__":
    main()
