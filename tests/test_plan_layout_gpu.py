"""The workspace layout of the plans with Winograd layers is the recorded one
(tests/golden/plan_layout.json; tests/test_plan_layout_host.py has the plans that need no device).

cilrs_net_create sets the Winograd kernels' attributes on the device, so these plans need one:
fp32 at batch 32 (layer1 on the Winograd kernel) and batch 128 (layers 1-3), both trunks, and
CILRS_WINO=2 at batch 4 in a child process (the switch is read once per process).  Nothing is
allocated and no kernel runs."""
import pytest

from test_plan_layout_host import FIXTURE, P

pytestmark = pytest.mark.gpu

GPU = [e for e in FIXTURE["plans"] if e["set"] == "gpu"]


def test_fixture_holds_every_gpu_plan():
    assert sorted(e["key"] for e in GPU) == sorted(P.key(p) for p in P.gpu_plans())
    assert len(GPU) == 5 and all(e["rec"]["wino"] > 0 for e in GPU)
    wino = {e["key"]: e["rec"]["wino"] for e in GPU}
    # ResNet-34: layer1 has 6 stride-1 3x3 convolutions, layers 1-3 have 6 + 7 + 11
    assert wino["variant 0 batch 32 88x200 flags 0"] == 6
    assert wino["variant 0 batch 128 88x200 flags 0"] == 24


@pytest.mark.parametrize("entry", GPU, ids=[e["key"] for e in GPU])
def test_layout_is_the_recorded_one(entry):
    assert P.record(entry["plan"]) == entry["rec"]
