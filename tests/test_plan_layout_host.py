"""The workspace layout of a plan is the recorded one (tests/golden/plan_layout.json, written by
tools/plan_layout.py from the public queries of the C API), for the plans that need no device.

The Bump allocator behind cilrs_net_create is sequential, so the visible offsets bracket the hidden
regions: status_offset lies behind the split-K scratch, the 16-bit arenas behind that, and
workspace_bytes is the end -- a change of any size shows.  A change that means to move the layout
re-records the fixture with the tool and says so.

Independently of the fixture: every reported region is 256-byte aligned and inside the workspace,
the activations / statistics / pool / argmax / head tensors do not overlap, and the constructor's
refusals keep their messages."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("plan_layout_tool",
                                                  os.path.join(ROOT, "tools", "plan_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = load_tool()
FIXTURE = P.load_fixture()
HOST = [e for e in FIXTURE["plans"] if e["set"] == "host"]


def _entry(key):
    return [e for e in FIXTURE["plans"] if e["key"] == key][0]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_fixture_holds_every_host_plan_and_the_parent_commits_anchors():
    assert sorted(e["key"] for e in HOST) == sorted(P.key(p) for p in P.host_plans())
    assert len(HOST) == 18
    for e in HOST:
        assert e["plan"] in P.host_plans() and e["rec"]["wino"] == 0
    # what the library of the commit before the plan-construction refactor reported
    a = _entry("variant 0 batch 1 88x200 flags 0")["rec"]
    assert (a["ws"], a["status"]) == (92097024, 44215552)
    b = _entry("variant 0 batch 3 17x17 flags 0")["rec"]
    assert (b["ws"], b["status"]) == (62764032, 20028416)
    assert _entry("variant 1 batch 128 88x200 flags 1")["rec"]["ws"] == 7078957056


@pytest.mark.parametrize("entry", HOST, ids=[e["key"] for e in HOST])
def test_layout_is_the_recorded_one(entry):
    assert P.record(entry["plan"]) == entry["rec"]


def regions(rec, plan):
    """(name, first byte, bytes, must be 256-byte aligned) of everything the queries report"""
    b = plan["batch"]
    feat, comb = rec["io"][4], rec["io"][3]
    out = [("status", rec["status"], 16, True), ("argmax", rec["argmax"][0], rec["argmax"][1], True),
           ("x4", rec["io"][0], 4 * rec["io"][1], True), ("combined", rec["io"][2], 4 * b * comb, True)]
    y, z, numel, _ = rec["act"][0]
    assert y == z
    out.append(("pool", 4 * y, 4 * numel, True))
    for ci, (y, z, numel, _) in enumerate(rec["act"][1:]):
        out += [("y%d" % ci, 4 * y, 4 * numel, True), ("z%d" % ci, 4 * z, 4 * numel, True)]
    for ci, (stats, ch, _, _) in enumerate(rec["bn"]):
        out.append(("stats%d" % ci, 4 * stats, 4 * 4 * ch, True))
    ncmd = len(rec["heads"]) // 6
    for which in range(6):
        for br in range(ncmd if which >= 4 else 1):
            off, rows, cols, ld = rec["heads"][which * ncmd + br]
            assert rows == b
            if which == 1:          # the speed columns of `combined`: reported above as a whole
                assert 4 * (off - feat) == rec["io"][2] and ld == comb
                continue
            assert ld == cols
            out.append(("head%d.%d" % (which, br), 4 * off, 4 * rows * ld, True))
    for ci, (w16, bias, numel, ch) in enumerate(rec["infer16"]):
        # (the arenas are aligned: the stem's pair and the first entries of the table)
        out += [("w16_%d" % ci, w16, 2 * numel, ci <= 1), ("bias16_%d" % ci, bias, 4 * ch, ci <= 1)]
    for i, (a, da, h, w, ch) in enumerate(rec["gradcam"]):
        out += [("cam_a%d" % (i + 1), 4 * a, 4 * b * h * w * ch, True),
                ("cam_da%d" % (i + 1), 4 * da, 4 * b * h * w * ch, True)]
    return out


@pytest.mark.parametrize("entry", HOST, ids=[e["key"] for e in HOST])
def test_regions_are_aligned_inside_the_workspace_and_disjoint(entry):
    rec = P.record(entry["plan"])
    regs = regions(rec, entry["plan"])
    assert rec["ws"] % 256 == 0
    for name, start, size, aligned in regs:
        assert size > 0 and start + size <= rec["ws"], name
        assert not aligned or start % 256 == 0, name
    # y, z, stats, pool, argmax and the heads' tensors: no two overlap
    own = sorted((s, s + n, name) for name, s, n, _ in regs
                 if name[0] in "yz" or name.startswith(("stats", "pool", "argmax", "head", "combined")))
    assert len(own) == 3 * len(rec["bn"]) + 3 + 3 + 2 * (len(rec["heads"]) // 6)
    for (_, end, name), (start, _, nxt) in zip(own, own[1:]):
        assert end <= start, (name, nxt)


def _refused(*args):
    lib = P.load_lib().lib()
    assert lib.cilrs_net_create_ex(*args) != 0
    return lib.cilrs_last_error().decode()


def test_constructor_refusals_keep_their_messages():
    net = C.c_void_p()
    assert _refused(0, 1, 88, 200, 0, None) == "cilrs_net_create: out is NULL"
    assert _refused(0, 1, 88, 200, 2, C.byref(net)) == "cilrs_net_create: unknown flags 0x2"
    assert _refused(7, 1, 88, 200, 0, C.byref(net)) == "cilrs_net_create: variant 7 out of range"
    assert _refused(0, 1, 16, 17, 0, C.byref(net)) == "cilrs_net_create: bad geometry 1 16 17"
    assert not net.value


def test_a_plan_with_winograd_layers_fails_cleanly_without_a_device():
    """cilrs_net_create sets the Winograd kernels' attributes at plan build; with no device that
    fails behind the allocation of the plan.  The library says why and the next create works."""
    L = P.load_lib()
    small = P.host_plans()[0]
    if not _has_gpu():
        net, err = P.create(L, {"variant": 0, "batch": 128, "h": 88, "w": 200, "flags": 0})
        assert net is None and "hipFuncSetAttribute" in err
    assert P.record(small) == _entry(P.key(small))["rec"]
