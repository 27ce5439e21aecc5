#!/usr/bin/env python3
"""Record what the public queries of the C API show of a plan's workspace layout.

    python tools/plan_layout.py record --plans host -o tests/golden/plan_layout.json
    python tools/plan_layout.py record --plans gpu  -o tests/golden/plan_layout.json
    CILRS_LIB=/path/to/other/libcilrs_hip.so python tools/plan_layout.py record ...

ctypes on the library alone (cilrs_mi355/_lib.py is loaded by file path: no torch, no device
memory, no launch).  `record` replaces the plans of the chosen set in the output file and keeps
the others.  The "host" plans need no GPU; the "gpu" plans have Winograd layers, whose kernel
attributes cilrs_net_create sets on the device.  A plan with an "env" entry is recorded by a child
process (the library reads its switches once per process).

tests/test_plan_layout_host.py and tests/test_plan_layout_gpu.py compare a fresh recording with the
fixture exactly.  The Bump allocator is sequential, so the offsets that are visible bracket the
regions that are not: a change of any size moves status_offset, the 16-bit arenas or
workspace_bytes.  A change that MEANS to move the layout re-records the fixture with this tool.
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_layout.json")

# what each array of a record holds, in order
FIELDS = {
    "ws": "cilrs_net_workspace_bytes",
    "status": "cilrs_net_status_offset",
    "act": "cilrs_net_activation_info, conv -1 then every conv: [y_offset, z_offset, numel, channels]",
    "bn": "cilrs_net_bn_layer_info, every conv: [stats_offset, channels, rows, bn_index]",
    "argmax": "cilrs_net_pool_argmax_info: [byte_offset, numel]",
    "heads": "cilrs_net_head_activation_info, which 0..5 x every branch: [offset, rows, cols, ld]",
    "infer16": "cilrs_net_infer16_conv_info, every conv: [w16_offset, bias_offset, w16_numel, channels]",
    "io": "cilrs_net_infer16_io_info: [x4_offset, x4_numel, combined_offset, combined_ld, features]",
    "gradcam": "cilrs_net_gradcam_info, layers 1..4: [a_offset, da_offset, h, w, channels]",
    "wino": "cilrs_net_wino_convs",
    "classes": "cilrs_net_conv_classes, every conv: [fwd, dgrad]",
}


def _plan(variant, batch, h, w, flags=0, env=None):
    return {"variant": variant, "batch": batch, "h": h, "w": w, "flags": flags, "env": env or {}}


def host_plans():
    """creatable without a device: no layer of these reaches the Winograd block-count rule (and
    the bf16 train plan has no Winograd layers at all)"""
    plans = [_plan(v, b, h, w, f) for v in (0, 1)
             for (b, h, w) in ((1, 88, 200), (2, 32, 32), (4, 88, 200), (3, 17, 17)) for f in (0, 1)]
    return plans + [_plan(v, 128, 88, 200, 1) for v in (0, 1)]


def gpu_plans():
    """fp32 train plans with Winograd layers: layer1 at batch 32, layers 1-3 at batch 128, every
    supported layer under CILRS_WINO=2"""
    plans = [_plan(v, b, 88, 200) for v in (0, 1) for b in (32, 128)]
    return plans + [_plan(0, 4, 88, 200, 0, {"CILRS_WINO": "2"})]


PLAN_SETS = {"host": host_plans, "gpu": gpu_plans}


def key(p):
    env = "".join(" %s=%s" % kv for kv in sorted(p["env"].items()))
    return "variant %d batch %d %dx%d flags %d%s" % (p["variant"], p["batch"], p["h"], p["w"],
                                                      p["flags"], env)


def load_lib():
    spec = importlib.util.spec_from_file_location(
        "_cilrs_lib", os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd", "cilrs_mi355", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def create(L, p):
    """(handle, None) or (None, the library's message)"""
    net = C.c_void_p()
    rc = L.lib().cilrs_net_create_ex(p["variant"], p["batch"], p["h"], p["w"], p["flags"], C.byref(net))
    if rc != 0:
        return None, (L.lib().cilrs_last_error() or b"").decode()
    return net, None


def describe(L, net, variant):
    lib = L.lib()
    nconv = lib.cilrs_variant_num_bn(variant)            # one BatchNorm per convolution
    ncmd = (variant >> 8) or 4

    def q(fn, *args, out):
        vals = [t() for t in out]
        L.check(fn(net, *args, *[C.byref(v) for v in vals]))
        return [v.value for v in vals]

    S, I = C.c_size_t, C.c_int
    return {
        "ws": lib.cilrs_net_workspace_bytes(net),
        "status": lib.cilrs_net_status_offset(net),
        "act": [q(lib.cilrs_net_activation_info, ci, out=(S, S, S, I)) for ci in range(-1, nconv)],
        "bn": [q(lib.cilrs_net_bn_layer_info, ci, out=(S, I, I, I)) for ci in range(nconv)],
        "argmax": q(lib.cilrs_net_pool_argmax_info, out=(S, S)),
        "heads": [q(lib.cilrs_net_head_activation_info, which, br, out=(S, I, I, I))
                  for which in range(6) for br in range(ncmd)],
        # (folded_half says what the arenas hold after a forward: not layout)
        "infer16": [q(lib.cilrs_net_infer16_conv_info, ci, out=(S, S, S, I, I))[:4] for ci in range(nconv)],
        "io": q(lib.cilrs_net_infer16_io_info, out=(S, S, S, I, I)),
        "gradcam": [q(lib.cilrs_net_gradcam_info, layer, out=(S, S, I, I, I)) for layer in range(1, 5)],
        "wino": lib.cilrs_net_wino_convs(net),
        "classes": [q(lib.cilrs_net_conv_classes, ci, out=(I, I)) for ci in range(nconv)],
    }


def record_one(p):
    """the record of one plan, in this process"""
    L = load_lib()
    net, err = create(L, p)
    if net is None:
        raise RuntimeError("%s: %s" % (key(p), err))
    try:
        return describe(L, net, p["variant"])
    finally:
        L.lib().cilrs_net_destroy(net)


def record(p):
    """the record of one plan; a plan with environment switches goes through a child process"""
    if not p["env"]:
        return record_one(p)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "one", json.dumps(p)],
                         env=dict(os.environ, **p["env"]), capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("%s: child exited %d: %s" % (key(p), out.returncode, out.stderr[-2000:]))
    return json.loads(out.stdout)


def load_fixture(path=FIXTURE):
    with open(path) as f:
        return json.load(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("record", help="record a set of plans into a fixture file")
    r.add_argument("--plans", choices=sorted(PLAN_SETS), required=True)
    r.add_argument("-o", "--out", default=FIXTURE)
    o = sub.add_parser("one", help="print the record of one plan (JSON), in this process")
    o.add_argument("plan")
    args = ap.parse_args()
    if args.cmd == "one":
        print(json.dumps(record_one(json.loads(args.plan))))
        return
    doc = load_fixture(args.out) if os.path.exists(args.out) else {"plans": []}
    kept = [e for e in doc["plans"] if e["set"] != args.plans]
    new = [{"key": key(p), "set": args.plans, "plan": p, "rec": record(p)} for p in PLAN_SETS[args.plans]()]
    doc = {"fields": FIELDS, "plans": sorted(kept + new, key=lambda e: (e["set"] != "host", e["key"]))}
    with open(args.out, "w") as f:
        f.write('{"fields":%s,\n"plans":[\n' % json.dumps(doc["fields"], separators=(",", ":")))
        f.write(",\n".join(json.dumps(e, separators=(",", ":")) for e in doc["plans"]))
        f.write("\n]}\n")
    for e in new:
        print("%-60s workspace %12d  status %12d  wino %d" % (e["key"], e["rec"]["ws"], e["rec"]["status"],
                                                               e["rec"]["wino"]))


if __name__ == "__main__":
    main()
