"""Host side of the saliency feature: what needs no GPU -- the new C-ABI entries are declared,
bound and exported, and Predictor.saliency's `output` argument is validated on the host."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("cilrs_net_backward_data", "cilrs_net_forward_frozen_u8",
               "cilrs_net_forward_frozen_camera", "cilrs_saliency_map", "cilrs_bn_bwd_frozen",
               "cilrs_bn_bwd_pool_frozen")


def test_new_entries_are_declared_bound_and_exported():
    from cilrs_mi355 import _lib as L
    header = open(os.path.join(ROOT, "include", "cilrs_hip.h")).read()
    lib = L.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in L.SIGNATURES
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    # backward_data takes cilrs_net_backward's arguments
    assert L.SIGNATURES["cilrs_net_backward_data"] == L.SIGNATURES["cilrs_net_backward"]


def test_saliency_output_argument():
    from cilrs_mi355.predict import Predictor
    w = Predictor._saliency_weights
    assert w("steer").tolist() == [1, 0, 0, 0] and w("throttle").tolist() == [0, 1, 0, 0]
    assert w("brake").tolist() == [0, 0, 1, 0] and w("speed").tolist() == [0, 0, 0, 1]
    got = w([0.5, 0, -1, 2])
    assert got.dtype == np.float32 and got.tolist() == [0.5, 0.0, -1.0, 2.0]
    for bad in ("steering", "", [1, 0, 0], [1, 0, 0, 0, 0], [[1, 0, 0, 0]], None,
                [1.0, float("nan"), 0, 0], ["a", "b", "c", "d"]):
        with pytest.raises(ValueError):
            w(bad)
