"""Host side of fine-tuning with a frozen trunk prefix: the freeze-state reader on a CILRS built on
the CPU (no engine), and the bucket plan of the data-parallel reducer with a cut (gloo)."""
import os

import pytest
import torch

GROUPS = ("stem", "layer1", "layer2", "layer3", "layer4")
N_CHILDREN = {1: 4, 2: 5, 3: 6, 4: 7, 5: 8}


def _model(resnet50=False):
    from cilrs_mi355 import CILRS, CILRSResNet50
    return (CILRSResNet50 if resnet50 else CILRS)(4, 0.0).train()


@pytest.mark.parametrize("resnet50", [False, True])
def test_freeze_state_reads_every_supported_cut(resnet50):
    m = _model(resnet50)
    assert m._engine is None
    assert m.freeze_state() == (0, 0)
    for k in range(1, 6):
        # torch's idiom: e == g == k
        m = _model(resnet50)
        prefix = m.visual_encoder[:N_CHILDREN[k]]
        prefix.eval()
        for p in prefix.parameters():
            p.requires_grad_(False)
        assert m.freeze_state() == (k, k)
        # requires_grad_(False) alone: e == 0, g == k
        m = _model(resnet50)
        for p in m.visual_encoder[:N_CHILDREN[k]].parameters():
            p.requires_grad_(False)
        assert m.freeze_state() == (0, k)
        # the convenience sets exactly the same flags
        m2 = _model(resnet50).freeze(GROUPS[k - 1])
        assert m2.freeze_state() == (k, k)
        ref = _model(resnet50)
        prefix = ref.visual_encoder[:N_CHILDREN[k]]
        prefix.eval()
        for p in prefix.parameters():
            p.requires_grad_(False)
        assert [p.requires_grad for p in m2.parameters()] == [p.requires_grad for p in ref.parameters()]
        flags = [(n, mod.training) for n, mod in m2.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)]
        assert flags == [(n, mod.training) for n, mod in ref.named_modules()
                         if isinstance(mod, torch.nn.BatchNorm2d)]
    assert m._engine is None


def test_freeze_unfreeze_and_train_interplay():
    m = _model()
    m.freeze("layer3")
    assert m.freeze_state() == (4, 4)
    m.freeze("layer1")                          # a shorter prefix: the groups behind it come back
    assert m.freeze_state() == (2, 2)
    m.unfreeze()
    assert m.freeze_state() == (0, 0)
    assert all(p.requires_grad for p in m.parameters())
    assert all(mod.training for mod in m.modules())
    m.freeze("layer2")
    m.train()                                   # as in torch: train() clears the eval flags ...
    assert m.freeze_state() == (0, 3)           # ... and leaves requires_grad alone
    m.freeze("layer2")
    m.eval()                                    # eval mode: no BatchNorm cut to speak of
    assert m.freeze_state() == (0, 3)
    m.freeze("layer4")                          # in eval mode freeze() keeps every module in eval
    assert not any(mod.training for mod in m.modules())
    m.train()
    assert m.freeze_state() == (0, 5)
    with pytest.raises(ValueError, match="freeze"):
        m.freeze("heads")


def _refusals():
    def behind(m):
        m.visual_encoder[6].requires_grad_(False)
    def inside(m):
        m.freeze("stem")
        m.visual_encoder[4][1].conv2.weight.requires_grad_(False)
    def head(m):
        m.speed_predictor[0].bias.requires_grad_(False)
    def branch(m):
        m.control_branches[2].requires_grad_(False)
    def e_gt_g(m):
        m.freeze("stem")
        m.visual_encoder[4].eval()
    def e_gt_g_none_frozen(m):
        m.visual_encoder[1].eval()
    def e_lt_g(m):
        m.freeze("layer2")
        m.visual_encoder[5].train()
    def bn_behind(m):
        m.visual_encoder[7][2].bn1.eval()
    def bn_partial(m):
        m.freeze("layer1")
        m.visual_encoder[4][0].bn2.train()
    return {"behind": (behind, "visual_encoder.6.0.conv1.weight"),
            "inside": (inside, "visual_encoder.4.1.conv2.weight"),
            "head": (head, "speed_predictor.0.bias"),
            "branch": (branch, "control_branches.2.0.weight"),
            "e_gt_g": (e_gt_g, "visual_encoder.4.0.bn1"),
            "e_gt_g_none_frozen": (e_gt_g_none_frozen, "visual_encoder.1"),
            "e_lt_g": (e_lt_g, "visual_encoder.5.0.bn1"),
            "bn_behind": (bn_behind, "visual_encoder.7.2.bn1"),
            "bn_partial": (bn_partial, "visual_encoder.4.0.bn2")}


@pytest.mark.parametrize("name", sorted(_refusals()))
def test_unsupported_patterns_name_the_offender(name):
    apply, named = _refusals()[name]
    m = _model()
    apply(m)
    with pytest.raises(RuntimeError, match=named.replace(".", r"\.")):
        m.freeze_state()


def test_lr_mult_rejects_unknown_groups():
    from cilrs_mi355 import CONFIG_A, TrainConfig
    from cilrs_mi355.train import GROUP_NAMES
    assert GROUP_NAMES == GROUPS + ("heads",)
    assert CONFIG_A.lr_mult is None
    cfg = TrainConfig(lr_mult={"layer5": 0.1})
    assert cfg.lr_mult == {"layer5": 0.1}        # (validated where it is used: Trainer.__init__)


def test_bucket_plan_with_a_cut():
    from cilrs_mi355.engine import group_ranges, segment_ranges
    from cilrs_mi355.parallel import bucket_plan
    segs = segment_ranges()
    groups = group_ranges()
    assert [b for b, _ in groups] == sorted(b for b, _ in groups) and groups[0][0] == 0
    assert all(groups[i][1] == groups[i + 1][0] for i in range(5))
    assert all(b % 4 == 0 for b, _ in groups)                    # 16-byte aligned starts
    full = bucket_plan(segs)
    assert bucket_plan(segs, 0) == full and len(full) == 3
    n = groups[5][1]
    for k in range(1, 6):
        plan = bucket_plan(segs, k)
        cut = groups[k][0]
        # trainable floats, each exactly once; nothing below the cut
        assert sorted((b, e) for _, b, e in plan)[0][0] == cut
        assert sum(e - b for _, b, e in plan) == n - cut
        assert all(b >= cut and last <= 5 - k for last, b, e in plan)
        assert len(plan) == {1: 3, 2: 3, 3: 2, 4: 1, 5: 1}[k]
    assert bucket_plan(segs, 3) == [full[0], full[1]]
    with pytest.raises(ValueError):
        bucket_plan(segs, 6)


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cilrs_mi355 import _lib as L
    from cilrs_mi355.engine import group_ranges
    from cilrs_mi355.parallel import BucketedAllReduce
    n = L.lib().cilrs_param_arena_floats()
    ok = True
    for k, want_calls, want_coll in ((2, [(0, 2), (2, 3), (3, 4)], 3), (3, [(0, 2), (2, 3)], 2),
                                     (5, [(0, 1)], 1), (0, [(0, 2), (2, 3), (3, 6)], 3)):
        flat = torch.full((n,), float(rank + 1))
        red = BucketedAllReduce(flat)

        class FakeEngine:
            def __init__(self):
                self.calls = []

            def run_backward(self, plan, dc, dp, a, b):
                self.calls.append((a, b))
        eng = FakeEngine()
        seen = []
        red.backward_and_reduce(eng, None, None, None, frozen_groups=k,
                                after_bucket=lambda i, b, e: seen.append((b, e)))
        cut = group_ranges()[k][0] if k else 0
        ok = ok and eng.calls == want_calls and red.collectives == want_coll == len(seen)
        # the frozen range is not reduced (still this rank's own values), the rest is summed
        ok = ok and bool((flat[:cut] == float(rank + 1)).all()) and bool((flat[cut:] == 3.0).all())
        ok = ok and all(b >= cut for b, _ in seen) and not red._pending
    q.put((rank, ok))
    dist.destroy_process_group()


def test_bucketed_allreduce_with_a_cut_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
    assert all(ok for _, ok in res), res
