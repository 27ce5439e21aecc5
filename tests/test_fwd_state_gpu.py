"""What may follow which forward on one plan (csrc/net.hip: cilrs_net::last, fwd_begin / fwd_commit).

One plan of the reference network at batch 1 on a 40x120 image -- the one geometry on which every
forward kind runs, the persistent launch and cilrs_net_forward_bn_stats (its smallest BatchNorm
still sees 8 rows) included.  For each "last forward" the table says which follow-up is accepted
and which is refused with which fragment of the message; the sequence cases below it cover what
one forward must not inherit from the one before.

Graph forwards run under weights key 0 ("unknown: never cache"): the cached graph is then replayed
whenever the pointers are the same, which is the only way a replay can follow a train-mode forward
(a caller that announces keys moves the key there, and the graph is captured again).
"""
import ctypes as C

import pytest
import torch

import cilrs_oracle as O

pytestmark = pytest.mark.gpu

B, H, W = 1, 40, 120
W_MIX = (0.75, -0.5, 0.25, 1.5)

BWD = "backward needs a preceding train-mode forward"
IG = "input_grads needs a preceding graph-keeping forward"
NO_BWD = "no matching backward"

_CACHE = {}


def _L():
    from cilrs_mi355 import _lib as L
    return L


class _Rig:
    """the model, its engine, the inputs and the scratch tensors every case shares"""

    def __init__(self):
        from cilrs_mi355 import CILRS
        torch.manual_seed(0)
        self.m = CILRS(4, 0.5).cuda()
        self.eng = self.m.engine()
        img, spd, cmd, _t, u8 = O.synthetic_batch(B, seed=5, h=H, w=W)
        self.img, self.spd, self.cmd = img.cuda(), spd.cuda(), cmd.cuda()
        self.u8 = torch.from_numpy(u8).cuda()
        self.dc = torch.tensor([W_MIX[:3]] * B, dtype=torch.float32, device="cuda")
        self.ds = torch.full((B,), W_MIX[3], dtype=torch.float32, device="cuda")
        self.dimage = torch.empty(B, 3, H, W, dtype=torch.float32, device="cuda")
        self.dspeed = torch.empty(B, dtype=torch.float32, device="cuda")
        n = self.eng.n_arena
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device="cuda")
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device="cuda")
        lib = _L().lib()
        self.bn_table = torch.zeros(lib.cilrs_variant_bn_stats_doubles(0), dtype=torch.float64,
                                    device="cuda")
        F = self.eng.feature_width()
        self.pivot = torch.zeros(F, dtype=torch.float32, device="cuda")
        self.moments = torch.zeros(lib.cilrs_feature_moments_doubles(F, 4), dtype=torch.float64,
                                   device="cuda")
        self.graph_out, self.old_outs = self.new_out(), []
        self.stream = torch.cuda.Stream()          # graph capture needs a non-default stream
        self.lane = 100
        torch.cuda.synchronize()                   # everything above was filled on the default stream

    def new_out(self):
        return (torch.empty(B, 3, dtype=torch.float32, device="cuda"),
                torch.empty(B, dtype=torch.float32, device="cuda"))

    def plan(self):
        return self.eng.plan(B, H, W)

    def fresh_plan(self):
        """a plan no forward has run on"""
        self.lane += 1
        pl = self.eng.plan(B, H, W, lane=self.lane)
        self.eng.last_plan = pl
        return pl

    # ---- the forwards ------------------------------------------------------------------------------
    def none(self):
        return self.fresh_plan()

    def eval_f32(self):
        self.eng.run_forward_u8(self.u8, self.spd, self.cmd)
        return self.plan()

    def eval_f16(self):
        self.eng.run_forward_u8(self.u8, self.spd, self.cmd, half=True)
        return self.plan()

    def b1(self):
        self.eng.run_forward_u8(self.u8, self.spd, self.cmd, persistent=True)
        return self.plan()

    def graph(self):
        """cilrs_net_forward_u8_graph under weights key 0: captured when an output pointer is new
        to the plan's cached graph, replayed when every pointer is the one it holds"""
        L = _L()
        pl = self.plan()
        out = self.graph_out
        L.check(L.lib().cilrs_net_set_weights_key(pl.handle, 0))
        L.check(L.lib().cilrs_net_forward_u8_graph(
            pl.handle, C.byref(pl.bufs), L.ptr(self.u8), L.ptr(self.spd), L.ptr(self.cmd),
            L.ptr(out[0]), L.ptr(out[1]), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.eng.last_plan = pl
        return pl

    def graph_capture(self):
        self.old_outs.append(self.graph_out)       # (kept, so that the new pointers are new)
        self.graph_out = self.new_out()
        return self.graph()

    def graph_replay(self):
        self.graph_capture()
        return self.graph()

    def train(self):
        return self.eng.run_forward(self.img, self.spd, self.cmd, True, 0.5, 1)[2]

    def ft22(self):
        return self.eng.run_forward_ft(self.img, self.spd, self.cmd, 2, 2, 0.5, 1)[2]

    def frozen(self):
        return self.eng.run_forward_frozen_u8(self.u8, self.spd, self.cmd)[2]

    def bn_stats(self):
        return self.eng.run_forward_bn_stats(self.img, self.bn_table)

    # ---- the follow-ups: None when accepted, the message when refused ---------------------------------
    @staticmethod
    def outcome(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except RuntimeError as e:
            return str(e)
        return None

    def backward(self, pl, seg, data_only=False):
        return self.outcome(self.eng.run_backward, pl, self.dc, self.ds, segments=seg,
                            data_only=data_only)

    def backward_step(self, pl):
        return self.outcome(self.eng.run_backward_step, pl, self.dc, self.ds, self.exp_avg,
                            self.exp_avg_sq, 0.0, (0.9, 0.999), 1e-8, 0.0, 1)

    def input_grads(self, pl, what):
        kw = {"dspeed": self.dspeed} if what == "dspeed" else {"dimage": self.dimage}
        return self.outcome(self.eng.run_input_grads, pl, **kw)

    def heads_mc(self):
        return self.outcome(self.eng.run_heads_mc, self.spd, self.cmd, 4, 0.5, seed=1)

    def gradcam(self, layer):
        return self.outcome(self.eng.run_gradcam, self.spd, self.cmd, W_MIX, layer=layer)

    def feature_moments(self):
        return self.outcome(self.eng.run_feature_moments, self.cmd, self.pivot, self.moments)

    def ft_cut(self, pl):
        L = _L()
        e, g = L.i32(), L.i32()
        L.check(L.lib().cilrs_net_ft_cut(pl.handle, C.byref(e), C.byref(g)))
        return e.value, g.value


@pytest.fixture
def rig():
    if "rig" not in _CACHE:
        _CACHE["rig"] = _Rig()
    r = _CACHE["rig"]
    with torch.cuda.stream(r.stream):
        yield r
        torch.cuda.synchronize()
    r.plan().check_status()


def _same(got, want, what):
    print(f"FWDSTATE {what}: {'accepted' if got is None else got}")
    if want is None:
        assert got is None, (what, got)
    else:
        assert got is not None and want in got, (what, want, got)


# what follows a forward that left nothing behind / an eval-mode forward / one that keeps its graph
_NONE = dict(bwd01=BWD, step=BWD, dspeed=IG, dimage=IG, mc="no forward", cam4="no forward",
             cam3="no forward", moments="no forward", cut=(0, 0))
_EVAL = dict(bwd01=BWD, step=BWD, dspeed=IG, dimage=IG, mc=None, cam4=None, cam3=NO_BWD,
             moments=None, cut=(0, 0))
_TRAIN = dict(bwd01=None, step=None, dspeed=None, dimage="dimage needs segment 5", mc="train mode",
              cam4="train mode", cam3="train mode", moments="train mode", cut=(0, 0))

# last forward: (the forward that runs before it, what each follow-up must answer)
TABLE = {
    "none": (None, _NONE),
    "eval_f32": ("frozen", _EVAL),
    "eval_f16": ("frozen", dict(_EVAL, cam4="16-bit", cam3="16-bit")),
    "b1": ("frozen", _EVAL),
    "graph_capture": ("frozen", _EVAL),
    "graph_replay": ("frozen", _EVAL),
    "train": ("ft22", _TRAIN),
    "ft22": ("frozen", dict(_TRAIN, step="froze", dimage="froze", cam4="fine-tuning",
                            cam3="fine-tuning", cut=(2, 2))),
    "frozen": ("ft22", dict(_TRAIN, mc=None, cam4=None, cam3=NO_BWD, moments=None)),
    "bn_stats": ("ft22", dict(_NONE, mc="train mode", cam4="train mode", cam3="train mode",
                              moments="train mode")),
}


@pytest.mark.parametrize("last", list(TABLE))
def test_what_may_follow(rig, last):
    """Each group of follow-ups starts from the forward under test, run anew behind a forward of
    another kind (a graph-keeping one before an eval-mode one and the reverse, a cut before the
    forwards that must clear it), so that nothing the row asserts is left over from the row before."""
    before, want = TABLE[last]

    def forward():
        if before:
            getattr(rig, before)()
        return getattr(rig, last)()

    pl = forward()
    _same(rig.backward(pl, (0, 1)), want["bwd01"], f"{last} -> backward [0,1)")
    _same(rig.input_grads(pl, "dspeed"), want["dspeed"], f"{last} -> backward -> input_grads(dspeed)")
    _same(rig.input_grads(pl, "dimage"), want["dimage"], f"{last} -> backward -> input_grads(dimage)")
    pl = forward()
    _same(rig.backward_step(pl), want["step"], f"{last} -> backward_step")
    pl = forward()
    _same(rig.heads_mc(), want["mc"], f"{last} -> heads_mc")
    _same(rig.gradcam(4), want["cam4"], f"{last} -> gradcam layer 4")
    _same(rig.gradcam(3), want["cam3"], f"{last} -> gradcam layer 3")
    _same(rig.feature_moments(), want["moments"], f"{last} -> feature_moments")
    assert rig.ft_cut(pl) == want["cut"], (last, rig.ft_cut(pl))


def test_gradcam_layer3_reads_the_backward_of_this_forward(rig):
    pl = rig.frozen()
    _same(rig.backward(pl, (0, 2), data_only=True), None, "frozen -> backward_data [0,2)")
    _same(rig.gradcam(3), None, "frozen -> backward_data [0,2) -> gradcam layer 3")
    # two calls that continue one another are one unbroken run
    pl = rig.frozen()
    _same(rig.backward(pl, (0, 1)), None, "frozen -> backward [0,1)")
    _same(rig.backward(pl, (1, 2)), None, "frozen -> backward [0,1) -> backward [1,2)")
    _same(rig.gradcam(3), None, "frozen -> backward [0,1) -> backward [1,2) -> gradcam layer 3")


@pytest.mark.parametrize("between", ["eval_f32", "b1", "graph_replay"])
def test_another_forward_in_between_breaks_the_run(rig, between):
    if between == "graph_replay":
        rig.graph_replay()                         # the graph is there: the call below replays it
        between = "graph"
    pl = rig.frozen()
    _same(rig.backward(pl, (0, 2), data_only=True), None, "frozen -> backward_data [0,2)")
    getattr(rig, between)()
    _same(rig.gradcam(3), NO_BWD, f"frozen -> backward_data [0,2) -> {between} -> gradcam layer 3")


@pytest.mark.parametrize("keeper", ["frozen", "train"])
def test_a_replayed_graph_ends_the_graph_keeping_forward(rig, keeper):
    """The replayed graph overwrites every z and the head activations and keeps no y and no
    max-pool argmax: nothing of the forward before it is left to differentiate."""
    rig.graph_replay()
    getattr(rig, keeper)()
    pl = rig.graph()                               # same pointers, key 0: a replay
    _same(rig.backward(pl, (0, 1)), BWD, f"{keeper} -> graph replay -> backward")
    _same(rig.input_grads(pl, "dspeed"), IG, f"{keeper} -> graph replay -> input_grads")


def test_the_cut_outlives_an_eval_forward_and_the_graph_does_not(rig):
    rig.ft22()
    pl = rig.eval_f32()
    assert rig.ft_cut(pl) == (2, 2)
    rig.frozen()
    pl = rig.eval_f32()
    _same(rig.input_grads(pl, "dspeed"), IG, "frozen -> eval -> input_grads(dspeed)")
    _same(rig.input_grads(pl, "dimage"), IG, "frozen -> eval -> input_grads(dimage)")
