"""The mask-matched gradient check (tests/_masked_grads.py) must fail when it should -- on the CPU,
a CPU realisation in place of the engine: the fp32 oracle on a channels_last image, which stores
the tensors the engine's accessors expose and computes its gradients from them.

The clean backend passes with R = 2 for both trunks; every sabotaged backend fails at the
sabotaged tensor -- and at the tensors upstream of it where the damage travels -- and nowhere
else; a backend whose STORED decisions are not its forward's fails the consistency conditions
before any gate is looked at.  Last, for the exact seeds and shapes of the GPU cases, the fp32
channels_last realisation stays inside every cap of step 3, so that the inputs are never the
reason a cap trips on the engine (no seed had to be changed for that).
"""
import pytest
import torch

import cilrs_oracle as O
import _masked_grads as M

R = 2
SMALL = M.case("host_2x40x72", B=2, H=40, W=72, seed=3, inputs=True)


def _trunk_names(orc):
    return [n for n, _ in orc.named_parameters() if n.startswith("visual_encoder.")]


def _fails(c, sabotage):
    with pytest.raises(M.GradFailure) as ei:
        M.check(M.CpuBackend(c, sabotage), c, R)
    assert not isinstance(ei.value, M.ConsistencyFailure), ei.value
    return ei.value.tensors()


@pytest.mark.parametrize("trunk,mode,e,B,H,W", [
    ("resnet34", "train", 0, 2, 40, 72), ("resnet34", "train", 0, 3, 34, 50),
    ("resnet50", "train", 0, 2, 40, 72), ("resnet50", "train", 0, 3, 34, 50),
    ("resnet34", "frozen", 0, 2, 40, 72), ("resnet34", "ft", 2, 2, 40, 72)])
def test_clean_backend_passes(trunk, mode, e, B, H, W):
    c = M.case(f"host_{trunk}_{mode}_{B}x{H}x{W}", mode=mode, e=e, trunk=trunk, B=B, H=H, W=W,
               seed=3, inputs=mode != "ft")
    res = M.check(M.CpuBackend(c), c, R)
    want = len(M.trainable_of(M.build_oracle(c), c)) + (2 if c["inputs"] else 0)
    assert res["rel"] <= M.CAP and len(res["rows"]) == want


def test_num_commands_other_than_four_goes_through_the_forced_forward():
    c = M.case("host_nc6", nc=6, B=6, H=40, W=72, seed=4)
    M.check(M.CpuBackend(c), c, R)


def test_one_weight_gradient_tap_zeroed():
    name = "visual_encoder.5.0.conv2.weight"
    assert _fails(SMALL, ("tap", name)) == [name]


def test_one_dbeta_off_by_a_thousandth():
    name = "visual_encoder.6.2.bn2.bias"
    assert _fails(SMALL, ("dbeta", name)) == [name]


def test_stale_relu_mask_in_the_backward():
    orc = M.build_oracle(SMALL)
    blk = orc.visual_encoder[6][1]
    conv = next(ci for ci, _, cv, _, _ in O.trunk_convs(orc) if cv is blk.conv1)
    trunk = _trunk_names(orc)
    last = trunk.index("visual_encoder.6.1.bn1.bias")
    # the layer's own three tensors, everything in front of them, and the image; nothing behind
    assert _fails(SMALL, ("stale", conv)) == sorted(trunk[:last + 1] + ["dimage"])


def test_one_pooling_window_moved_in_the_backward():
    # (d beta of the stem's BatchNorm is the plain sum of the scattered gradient: moving one
    #  element to a neighbour leaves it where it was, so that tensor rightly passes)
    assert _fails(SMALL, ("pool", None)) == ["dimage", "visual_encoder.0.weight",
                                             "visual_encoder.1.weight"]


def test_one_head_mask_column_dropped():
    k = int(M.inputs_of(SMALL)[2][0])
    orc = M.build_oracle(SMALL)
    # branch k's first layer reads the masked gradient; `combined` carries it on to the trunk and
    # -- through its speed columns -- to the speed encoder, which is upstream of every branch too
    want = _trunk_names(orc) + [f"control_branches.{k}.0.weight", f"control_branches.{k}.0.bias",
                                "dimage", "dspeed"] + \
        [n for n, _ in orc.named_parameters() if n.startswith("speed_encoder.")]
    assert _fails(SMALL, ("head", f"h1.{k}")) == sorted(want)


def test_stored_sign_wrong_fails_consistency_not_the_gates():
    orc = M.build_oracle(SMALL)
    conv = next(ci for ci, _, cv, _, _ in O.trunk_convs(orc) if cv is orc.visual_encoder[5][2].conv2)
    with pytest.raises(M.ConsistencyFailure) as ei:
        M.check(M.CpuBackend(SMALL, ("sign", conv)), SMALL, R)
    assert f"relu {conv}" in ei.value.tensors()


# (the two child-process cases run the inputs of train_b8 under other library switches)
_OWN_INPUTS = [c for c in M.GPU_CASES if not c["env"]]


@pytest.mark.parametrize("c", _OWN_INPUTS, ids=[c["name"] for c in _OWN_INPUTS])
def test_gpu_case_inputs_stay_inside_the_caps(c):
    M.check_caps(M.CpuBackend(c), c)
