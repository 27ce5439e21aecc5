"""The fp32 backward pass of the HIP engine against the mask-matched float64 oracle
(tests/_masked_grads.py has the method, the consistency conditions and the gates): the engine's own
ReLU, max-pool and BatchNorm-mode decisions are read back through the C-ABI's test accessors and
forced on the float64 oracle, so the two gradients differ by rounding alone and every tensor is
gated at R x the fp32 CPU oracle's own distance from float64 -- no percentile, no flip branch.

The cases (_masked_grads.GPU_CASES) are the smallest that reach each backward kernel family:
  train_b8              (8,88,200), the golden batch: implicit-GEMM data gradients with split-K,
                        Winograd-domain weight gradients, the stem weight-gradient kernel's served
                        geometry, the fused BatchNorm + ReLU + max-pool backward
  train_b3_odd          (3,90,202): odd maps at every level (45x101 -> 3x7), ragged tiles, the
                        general stem weight-gradient path
  train_b1              (1,88,200): batch statistics over one frame, M = 21 rows at layer4
  train_b32             (32,88,200): the default plan's Winograd forward / data gradient (with
                        tail) on layer1 -- wino_convs() > 0 asserted
  train_b8_wino         child process, CILRS_WINO=2: all 24 stride-1 3x3 layers on the Winograd
                        kernels, the channel-split launch of an under-filled layer included
  train_b8_wino_serial  child process, CILRS_WINO=2 CILRS_OVERLAP=0: the data-gradient tail
                        launches with their BatchNorm-backward partials
  frozen_b4             frozen graph (4,88,200): fixed-statistics BatchNorm backward on running
                        statistics off 0 / 1; parameters, dimage and dspeed
  ft3_b8                fine-tuning cut e = g = 3: eval-mode prefix with folded epilogues, backward
                        stops at the cut, trainable tensors only
  resnet50_b4           ResNet-50 (4,64,64): Bottleneck blocks, 1x1 and 2048-wide layers
  nc6_b12               num_commands = 6 (12,64,64): grouped head gradients, two rows per branch
  resnet50_b3_odd       ResNet-50 (3,90,202): train_b3_odd's odd maps (45x101 -> 3x7) through
                        Bottleneck blocks -- ragged tiles of the 1x1 and 2048-wide layers, stride-2
                        parity classes of different sizes

R: MEASURED_RATIOS below are the largest e_hip / max(e_cpu, floor) per case on an MI355X (L2 and
element), kept with the report line in profiles/masked_grad_floor.log; R = twice the largest of
them, rounded up.  The engine is bit-deterministic, so the ratios do not move from run to run; the
factor leaves room for a legal change of summation order.  Independently of R no tensor may be
further than 1e-4 (relative L2) from the forced float64 gradient (_masked_grads.CAP).
"""
import json
import math
import os
import subprocess
import sys

import pytest

import _masked_grads as M

pytestmark = pytest.mark.gpu

# case: (worst L2 ratio, worst element ratio, worst relative L2 error) as measured
MEASURED_RATIOS = {
    "train_b8": (1.349, 1.584, 4.23e-06),
    "train_b3_odd": (1.273, 1.587, 3.95e-06),
    "train_b1": (1.135, 1.558, 4.64e-06),
    "train_b32": (1.539, 2.166, 4.61e-06),         # 2.166: visual_encoder.5.0.bn2.bias, 6 Winograd layers
    "train_b8_wino": (1.164, 1.428, 3.80e-06),
    "train_b8_wino_serial": (1.164, 1.428, 3.80e-06),
    "frozen_b4": (1.441, 1.933, 5.60e-07),
    "ft3_b8": (1.303, 1.865, 2.79e-06),
    "resnet50_b4": (1.114, 1.489, 1.41e-05),       # 1.41e-5: visual_encoder.7.2.conv3.weight, CPU 1.4e-5 too
    "nc6_b12": (1.255, 1.519, 3.73e-06),
    "resnet50_b3_odd": (1.188, 1.510, 1.21e-05),   # 1.21e-5: visual_encoder.7.2.conv3.weight again
}
R = 5           # ceil(2 x 2.166)

_CASES = {c["name"]: c for c in M.GPU_CASES}
_SEEN = {}


def _run(name):
    c = _CASES[name]
    be = M.EngineBackend(c)
    res = M.check(be, c, R)
    _SEEN[name] = (res["l2"], res["elem"], res["rel"])
    return be, res


@pytest.mark.parametrize("name", ["train_b8", "train_b3_odd", "train_b1", "resnet50_b4", "nc6_b12",
                                  "resnet50_b3_odd"])
def test_train_mode_gradients(name):
    _run(name)


def test_train_b32_default_plan_winograd():
    be, _ = _run("train_b32")
    print(f"MASKED train_b32: {be.wino_convs()} convolutions on the Winograd kernels")
    assert be.wino_convs() > 0


def test_frozen_graph_parameters_and_input_gradients():
    c = _CASES["frozen_b4"]
    bns = [m for m in M.build_oracle(c).modules() if hasattr(m, "running_var")]
    assert all(float(m.running_mean.abs().max()) > 0.05 and float((m.running_var - 1).abs().max()) > 0.1
               for m in bns), "running statistics still at 0 / 1"
    _, res = _run("frozen_b4")
    assert {"dimage", "dspeed"} <= {r["name"] for r in res["rows"]}


def test_fine_tuning_cut_trainable_tensors_only():
    be, res = _run("ft3_b8")
    names = {r["name"] for r in res["rows"]}
    assert not any(n.startswith(("visual_encoder.0.", "visual_encoder.1.", "visual_encoder.4.",
                                 "visual_encoder.5.")) for n in names)
    assert "visual_encoder.6.0.conv1.weight" in names
    # the backward stopped at the cut: the frozen range of the gradient arena was not written
    cut = be.eng.trainable_begin(3)
    assert float(be.eng.grads[:cut].abs().max()) == 0.0


_CHILD = r"""
import sys, json
for p in sys.argv[1:4]:
    sys.path.insert(0, p)
import _masked_grads as M
c = next(c for c in M.GPU_CASES if c["name"] == sys.argv[4])
R = json.loads(sys.argv[5])
be = M.EngineBackend(c)
out = {"wino": be.wino_convs(), "failures": [], "kind": None}
try:
    res = M.check(be, c, R)
    out.update(l2=res["l2"], elem=res["elem"], rel=res["rel"])
except M.GradFailure as exc:
    out.update(failures=exc.failures, kind=type(exc).__name__)
print("RESULT " + json.dumps(out))
"""


def _child(name):
    """check() in a fresh child process under the case's library switches (they are read once per
    process); one child per test, nothing is started after an abnormal exit or a timeout."""
    c = _CASES[name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.update(c["env"])
    r = subprocess.run([sys.executable, "-c", _CHILD,
                        os.path.join(root, "cilrs-autonomous-driving-carla_amd"),
                        os.path.join(root, "oracle"), os.path.join(root, "tests"), name,
                        json.dumps(R)],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert not out["failures"], (out["kind"], out["failures"])
    _SEEN[name] = (out["l2"], out["elem"], out["rel"])
    return out


def test_all_winograd_layers_in_a_child_process():
    assert _child("train_b8_wino")["wino"] == 24


def test_winograd_tail_launches_without_overlap_in_a_child_process():
    assert _child("train_b8_wino_serial")["wino"] == 24


def test_masked_grads_report():
    """Runs last in this file: the figures MEASURED_RATIOS and profiles/masked_grad_floor.log
    record, and R against the rule that derives it from them."""
    worst = 0.0
    for name, (l2, el, rel) in _SEEN.items():
        print(f"MASKED REPORT {name}: worst L2 ratio {l2:.3f}, worst element ratio {el:.3f}, "
              f"worst relative L2 error {rel:.3e}")
        worst = max(worst, l2, el)
    print(f"MASKED REPORT largest ratio {worst:.3f} over {len(_SEEN)} cases; R {R}; cap {M.CAP:.0e}")
    rec = max(max(v[0], v[1]) for v in MEASURED_RATIOS.values())
    assert R == math.ceil(2 * rec), (R, rec)
