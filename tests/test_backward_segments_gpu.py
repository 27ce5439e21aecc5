"""A backward pass issued as several calls over consecutive segment ranges gives the same bits as
one call over all six segments (0 heads, 1..4 layer4..layer1, 5 stem).

The data-parallel bucket hooks (cilrs_mi355/parallel.py) and Grad-CAM rely on this: they stop the
pass between segments and continue it later.  What has to survive such a stop is the state the
pass keeps between its launches (net.hip cilrs_net::bwd: the dy ring's position, the side stream's
pending readers); what must not cross it is anything a call keeps to itself (BwdPass, the
BatchNorm partials a block hands to the one below).

Every case runs one forward and then Engine.run_backward under three partitions -- one call, six
calls of one segment, two calls of three -- each on a freshly built model with the same weights and
inputs, so BatchNorm buffers and the gradient arena start alike.  Every comparison is exact.

Sizes: batch 4 at 88x200 (layer4's maps are the 3x7 ones the position classes exist for) and
batch 2 at 32x32 (layer4 is a 1x1 map, a BatchNorm there sees two values per channel).
"""
import os
import subprocess
import sys

import pytest
import torch

import cilrs_oracle as O

pytestmark = pytest.mark.gpu

SIZES = {"b4_88x200": (4, 88, 200), "b2_32x32": (2, 32, 32)}
PARTITIONS = (
    ((0, 6),),
    tuple((i, i + 1) for i in range(6)),
    ((0, 3), (3, 6)),
)
CASES = ("fp32", "bf16", "resnet50", "ft2", "frozen_data_only")


def _model(case):
    from cilrs_mi355 import CILRS, CILRSResNet50
    m = (CILRSResNet50 if case == "resnet50" else CILRS)(num_commands=4, dropout=0.0)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), 5), strict=True)
    return m.cuda()


def _run(case, size, partition):
    """One fresh model, one forward, the backward in the calls of `partition`; what the case
    compares, as a dict of CPU tensors."""
    b, h, w = SIZES[size]
    img, spd, cmd, tgt, _ = O.synthetic_batch(b, seed=61, h=h, w=w)
    img, spd, cmd, tgt = (t.cuda() for t in (img, spd, cmd, tgt))
    m = _model(case)
    eng = m.engine()
    if case == "frozen_data_only":
        m.eval()
        ctl, ps, pl = eng.run_forward_frozen(img, spd, cmd)
    elif case == "ft2":
        m.train()
        ctl, ps, pl = eng.run_forward_ft(img, spd, cmd, 2, 2, 0.0, 0)
    else:
        m.train()
        if case == "bf16":
            eng.train_precision = "bf16"
        ctl, ps, pl = eng.run_forward(img, spd, cmd, True, 0.0, 0)
    # output gradients that do not depend on the forward: the batch's targets and speeds
    dc, dp = tgt.contiguous(), spd.contiguous()
    data_only = case == "frozen_data_only"
    for seg in partition:
        eng.run_backward(pl, dc, dp, segments=seg, data_only=data_only)
    out = {"controls": ctl, "pred_speed": ps}
    if data_only:
        dimage = torch.empty(b, 3, h, w, device=eng.device)
        dspeed = torch.empty(b, device=eng.device)
        eng.run_input_grads(pl, dimage, dspeed)
        out.update(dimage=dimage, dspeed=dspeed)
    else:
        out.update(grads=eng.grads, bn=eng.bn)
    torch.cuda.synchronize()
    pl.check_status()
    return {k: v.detach().cpu().clone() for k, v in out.items()}, eng, pl


def _check(case, size, need_winograd=False):
    """The three partitions of one case at one size; returns the plan's Winograd layer count."""
    ref, eng, pl = _run(case, size, PARTITIONS[0])
    wino = pl.wino_convs()
    if need_winograd:
        assert wino > 0, "no convolution of this plan is on the Winograd kernels"
    key = "dimage" if case == "frozen_data_only" else "grads"
    assert float(ref[key].abs().max()) > 0.0 and bool(torch.isfinite(ref[key]).all())
    if case == "ft2":
        # segments 4 and 5 run nothing: the frozen range of the arena was never written
        cut = eng.trainable_begin(2)
        assert float(ref["grads"][:cut].abs().max()) == 0.0
        assert float(ref["grads"][cut:].abs().max()) > 0.0
    for part in PARTITIONS[1:]:
        got, _, _ = _run(case, size, part)
        assert got.keys() == ref.keys()
        for k in ref:
            assert torch.equal(got[k], ref[k]), (case, size, part, k)
    return wino


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", CASES)
def test_partitioned_backward_equals_one_call(case, size):
    _check(case, size)


_CHILD = r"""
import sys
for p in sys.argv[1:4]:
    sys.path.insert(0, p)
import test_backward_segments_gpu as T
print("RESULT wino", T.child_winograd(sys.argv[4]))
"""


def child_winograd(size):
    """Runs in the child: the fp32 case with every stride-1 3x3 layer on the Winograd forward and
    data-gradient route; the plan must say so before anything is compared."""
    return _check("fp32", size, need_winograd=True)


@pytest.mark.parametrize("size", list(SIZES))
def test_partitioned_backward_on_the_winograd_route_in_a_child_process(size):
    """CILRS_WINO is read once per process, so the case runs in a fresh child started with
    CILRS_WINO=2 (one child per test, nothing is started after an abnormal exit or a timeout)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["CILRS_WINO"] = "2"
    r = subprocess.run([sys.executable, "-c", _CHILD,
                        os.path.join(root, "cilrs-autonomous-driving-carla_amd"),
                        os.path.join(root, "oracle"), os.path.join(root, "tests"), size],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT wino ")][-1]
    assert int(line.split()[-1]) > 0
