"""Host side of the implicit GEMM's position classes: the decision is a function of the shape (and
the split-K scratch) alone and needs no GPU -- cilrs_conv2d_takes_classes makes no launch."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd")
NEW_ENTRIES = ("cilrs_conv2d_fwd_stats", "cilrs_conv2d_dgrad_bnbwd", "cilrs_conv2d_takes_classes",
               "cilrs_net_conv_classes", "cilrs_conv2d_plan_info")
BIG = 1 << 28          # floats of split-K scratch: enough for every split the model considers


def _takes(N, H, W, Cin, Cout, K=3, stride=1, pad=1, dgrad=0, scratch=BIG, splitk=0):
    from cilrs_mi355 import _lib as L
    return L.lib().cilrs_conv2d_takes_classes(N, H, W, Cin, Cout, K, stride, pad, dgrad, scratch, splitk)


def test_new_entries_are_declared_bound_and_exported():
    from cilrs_mi355 import _lib as L
    header = open(os.path.join(ROOT, "include", "cilrs_hip.h")).read()
    lib = L.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in L.SIGNATURES
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]


def test_layer4_takes_classes_at_batch_128_only_with_whole_tiles_of_rows():
    for dgrad in (0, 1):
        assert _takes(128, 3, 7, 512, 512, dgrad=dgrad) == 1
        assert _takes(128, 3, 7, 512, 512, dgrad=dgrad, scratch=0) == 1     # shorter K loops pay unsplit too
        assert _takes(64, 3, 7, 512, 512, dgrad=dgrad) == 1                 # a corner class = one tile
        assert _takes(63, 3, 7, 512, 512, dgrad=dgrad) == 0                 # a corner class < 64 rows
        assert _takes(1, 3, 7, 512, 512, dgrad=dgrad) == 0                  # single frame: untouched
        assert _takes(7, 3, 7, 512, 512, dgrad=dgrad) == 0


def test_only_padded_stride_1_problems_have_classes():
    assert _takes(128, 3, 7, 512, 512, K=1, pad=0) == 0          # 1x1: no padding
    assert _takes(128, 6, 13, 256, 512, stride=2) == 0           # stride 2 (parity classes instead)
    assert _takes(128, 3, 7, 512, 512, K=3, pad=0) == 0          # valid convolution: every tap inside
    assert _takes(128, 3, 7, 4, 64) == 0                         # generic-tap path (Cin % 32 != 0)
    # the degenerate maps of the GPU tests: 1x7 (three classes), 2x2 (four corners), 6x13 (nine)
    assert _takes(64, 1, 7, 64, 64, scratch=0) == 1
    assert _takes(64, 2, 2, 64, 64, scratch=0) == 1
    assert _takes(64, 6, 13, 64, 64, scratch=0) == 1
    # a 5x5 filter: more taps (and more runs of columns) than a class launch holds
    assert _takes(64, 3, 7, 64, 64, K=5, pad=2) == 0


def _plan(N, H, W, Cin, Cout, K, stride, pad, dgrad, scratch=BIG, cfg=-1, splitk=0):
    import ctypes as C
    from cilrs_mi355 import _lib as L
    out = [C.c_int(-9) for _ in range(4)]
    L.check(L.lib().cilrs_conv2d_plan_info(N, H, W, Cin, Cout, K, stride, pad, dgrad, scratch, cfg,
                                           splitk, *[C.byref(v) for v in out]))
    return tuple(v.value for v in out)            # cfg, splitk, class_tiles, parity_fused


def test_plan_info_agrees_with_takes_classes_and_honours_forced_values():
    for dgrad in (0, 1):
        for N in (128, 64, 63, 7):
            cfg, splitk, tiles, parity = _plan(N, 3, 7, 512, 512, 3, 1, 1, dgrad)
            assert (tiles > 0) == bool(_takes(N, 3, 7, 512, 512, dgrad=dgrad)) and parity == -1
            assert tiles == 0 or cfg == 2             # classes run on the 64x64 tile
        assert _plan(5, 6, 13, 1024, 256, 1, 1, 0, dgrad, cfg=1, splitk=3)[:2] == (1, 3)
        assert _plan(5, 6, 13, 1024, 256, 1, 1, 0, dgrad, scratch=0)[1] == 1      # no scratch: no split
        assert _plan(128, 3, 7, 512, 512, 3, 1, 1, dgrad, cfg=-2)[2] == 0          # classes off for the call


def test_plan_info_parity_launches_of_a_stride_2_data_gradient():
    """one launch while cdiv(N * ceil(H/2) * ceil(W/2), 64) * (Cin / 64) < 1280; never under a forced
    tile or split; the forward of the same convolution has no parity classes"""
    assert _plan(8, 101, 99, 256, 256, 3, 2, 1, 1)[3] == 1          # 319 x 4 = 1,276 tiles
    assert _plan(8, 101, 103, 256, 256, 3, 2, 1, 1)[3] == 0         # 332 x 4 = 1,328
    assert _plan(2, 22, 50, 256, 512, 1, 2, 0, 1) == (2, 1, 0, 1)
    assert _plan(2, 22, 50, 256, 512, 1, 2, 0, 1, cfg=1, splitk=1) == (1, 1, 0, 0)
    assert _plan(2, 22, 50, 256, 512, 1, 2, 0, 1, splitk=2)[1:] == (2, 0, 0)
    assert _plan(8, 101, 103, 256, 256, 3, 2, 1, 0)[3] == -1


def test_environment_switch_turns_classes_off():
    code = ("import sys; sys.path.insert(0, %r); from cilrs_mi355 import _lib as L; "
            "print(L.lib().cilrs_conv2d_takes_classes(128, 3, 7, 512, 512, 3, 1, 1, 0, 1 << 28, 0))" % PKG)
    for value, want in (("0", "0"), ("1", "1")):
        env = dict(os.environ, CILRS_IGEMM_CLASSES=value)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                             check=True).stdout.strip()
        assert out == want, (value, out)
