"""``CILRS`` -- drop-in for the reference's nn.Module of the same name.

Mirrors model/autonomous_drive.py:361-399 (== notebook/notebook.ipynb:440-477):

* ctor ``CILRS(num_commands=4, dropout=p)``;
* ``forward(image f32[B,3,H,W], speed f32[B], command i64[B]) -> (controls f32[B,3],
  pred_speed f32[B])`` -- a 2-tuple, exactly what ``predict_controls`` (:915-917) and
  ``train_one_epoch`` (nb:549) unpack;
* the strict ``state_dict`` contract (:497): 250 entries, same names / logical shapes / dtypes.

The module tree holds ordinary ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.Linear`` objects purely
as parameter containers; none of their ``forward`` methods ever runs.  All arithmetic happens in
libcilrs_hip.so (hand-written gfx950 kernels) through :mod:`cilrs_mi355.engine`; on a device
without the HIP engine ``forward`` raises -- there is no eager/CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .engine import Engine


class _NoEagerForward(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError("cilrs_mi355 modules are parameter containers; call CILRS.forward, "
                           "which runs the HIP engine (no eager fallback)")


class BasicBlock(_NoEagerForward):
    """Parameter container with torchvision BasicBlock's attribute names."""

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride


class Bottleneck(_NoEagerForward):
    """Parameter container with torchvision Bottleneck's attribute names (ResNet-50 variant)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, 1, 0, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)      # stride on the 3x3
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, 1, 0, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


def _make_bottleneck_layer(inplanes, planes, blocks, stride):
    down = None
    if stride != 1 or inplanes != planes * 4:
        down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False),
                             nn.BatchNorm2d(planes * 4))
    layers = [Bottleneck(inplanes, planes, stride, down)]
    layers += [Bottleneck(planes * 4, planes) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


def _make_layer(inplanes, planes, blocks, stride):
    down = None
    if stride != 1 or inplanes != planes:
        down = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False),
                             nn.BatchNorm2d(planes))
    layers = [BasicBlock(inplanes, planes, stride, down)]
    layers += [BasicBlock(planes, planes) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


# trunk groups a fine-tuning run freezes, in order, and where they sit in `visual_encoder`
TRUNK_GROUPS = ("stem", "layer1", "layer2", "layer3", "layer4")
_GROUP_CHILDREN = ((0, 1), (4,), (5,), (6,), (7,))


class CILRS(nn.Module):
    VARIANT = 0          # engine architecture variant (include/cilrs_hip.h)
    FEATURES = 512

    def _trunk(self):
        # ResNet-34 trunk, re-wrapped exactly as autonomous_drive.py:366-370 does, so indices
        # 0,1,4,5,6,7 carry the parameters and 2,3,8,9 carry none.
        return nn.Sequential(
            nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.MaxPool2d(3, 2, 1),
            _make_layer(64, 64, 3, 1), _make_layer(64, 128, 4, 2),
            _make_layer(128, 256, 6, 2), _make_layer(256, 512, 3, 2),
            nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten())

    def __init__(self, num_commands=4, dropout=0.0):
        super().__init__()
        # generic like the reference's ctor (autonomous_drive.py:362, 380-381); every caller of the
        # reference passes 4.  The engine lays its arena out per plan for 1..8 branches; the
        # single-launch persistent frame kernel and the evaluation report exist for 4 only.
        if not (isinstance(num_commands, int) and 1 <= num_commands <= 8):
            raise ValueError("num_commands must be an integer in 1..8")
        self.num_commands = num_commands
        self.dropout = float(dropout)
        self.visual_encoder = self._trunk()
        feat = self.FEATURES
        self.speed_encoder = nn.Sequential(
            nn.Linear(1, 128), nn.ReLU(inplace=True), nn.Dropout(dropout),
            nn.Linear(128, 128), nn.ReLU(inplace=True))
        self.control_branches = nn.ModuleList([
            nn.Sequential(
                nn.Linear(feat + 128, 256), nn.ReLU(inplace=True), nn.Dropout(dropout),
                nn.Linear(256, 256), nn.ReLU(inplace=True), nn.Dropout(dropout),
                nn.Linear(256, 3))
            for _ in range(num_commands)])
        self.speed_predictor = nn.Sequential(
            nn.Linear(feat, 256), nn.ReLU(inplace=True), nn.Dropout(dropout),
            nn.Linear(256, 256), nn.ReLU(inplace=True),
            nn.Linear(256, 1))
        # torchvision.models.resnet34(pretrained=False) initialisation (:365)
        for m in self.visual_encoder.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self._engine = None
        self._dropout_calls = 0
        # anything that may rewrite parameters / buffers invalidates what the engine derived
        # from them for inference (engine.weights_key)
        self.register_load_state_dict_post_hook(lambda module, _keys: module.weights_changed())

    _live = None          # weak set of modules with an engine (global optimizer hook below)

    def weights_changed(self):
        """Tell the engine that parameters or BatchNorm buffers were modified in place (it then
        re-derives its cached inference state: folded BatchNorm scale/shift, 16-bit weights).
        Called automatically by load_state_dict, by train()/eval() switches and by the engine's
        own training kernels; needed only after other in-place edits made in eval mode."""
        if self._engine is not None:
            self._engine.weights_epoch += 1

    def train(self, mode=True):
        if mode != self.training:
            self.weights_changed()
        return super().train(mode)

    # -- fine-tuning: a frozen prefix of the trunk ---------------------------------------------
    def _freeze_lists(self):
        """Per trunk group: [(name, parameter)], [(name, BatchNorm2d)]; then the heads' parameters."""
        lists = self.__dict__.get("_ft_lists")
        if lists is None:
            groups = []
            for children in _GROUP_CHILDREN:
                ps, bns = [], []
                for ci in children:
                    child, prefix = self.visual_encoder[ci], f"visual_encoder.{ci}"
                    ps += [(f"{prefix}.{n}", p) for n, p in child.named_parameters()]
                    bns += [(f"{prefix}.{n}" if n else prefix, m) for n, m in child.named_modules()
                            if isinstance(m, nn.BatchNorm2d)]
                groups.append((ps, bns))
            heads = [(n, p) for n, p in self.named_parameters()
                     if not n.startswith("visual_encoder.")]
            lists = (groups, heads)
            self.__dict__["_ft_lists"] = lists
        return lists

    def freeze_state(self):
        """(e, g), read from the module's own flags on every step: g = leading trunk groups
        (stem, layer1 .. layer4) whose parameters all have requires_grad == False; e = leading
        groups whose BatchNorm2d modules are all in eval mode while the model is in train mode (0
        in eval mode).  Supported: e == g (torch's idiom: ``prefix.eval()`` +
        ``requires_grad_(False)``) and e == 0 (``requires_grad_(False)`` alone: batch statistics
        and moving running buffers in the prefix, as in torch).  Anything else raises a
        RuntimeError that names the first offending parameter or module -- a pattern the engine
        cannot honour must never silently train in full."""
        groups, heads = self._freeze_lists()
        g = 0
        for ps, _ in groups:
            if any(p.requires_grad for _, p in ps):
                break
            g += 1
        for gi in range(g, len(groups)):
            ps = groups[gi][0]
            frozen = [n for n, p in ps if not p.requires_grad]
            if not frozen:
                continue
            if gi == g:
                live = next(n for n, p in ps if p.requires_grad)
                raise RuntimeError(
                    f"CILRS fine-tuning: {frozen[0]} is frozen (requires_grad=False) but {live}, "
                    f"in the same group ({TRUNK_GROUPS[gi]}), is trainable; a group is frozen as a "
                    f"whole (CILRS.freeze)")
            raise RuntimeError(
                f"CILRS fine-tuning: {frozen[0]} is frozen (requires_grad=False) behind the "
                f"trainable group {TRUNK_GROUPS[g]}; only a leading prefix of the trunk can be "
                f"frozen (CILRS.freeze)")
        for n, p in heads:
            if not p.requires_grad:
                raise RuntimeError(
                    f"CILRS fine-tuning: {n} is frozen (requires_grad=False); freezing heads or "
                    f"single branches is not supported, only a leading prefix of the trunk")
        if not self.training:
            return 0, g
        e = 0
        for _, bns in groups:
            if any(m.training for _, m in bns):
                break
            e += 1
        for gi in range(e, len(groups)):
            stopped = [n for n, m in groups[gi][1] if not m.training]
            if stopped:
                live = next(n for n, m in groups[e][1] if m.training)
                why = (f"{live}, in the same group ({TRUNK_GROUPS[e]}), is in train mode" if gi == e
                       else f"{live}, in the group {TRUNK_GROUPS[e]} in front of it, is in train mode")
                raise RuntimeError(
                    f"CILRS fine-tuning: BatchNorm {stopped[0]} is in eval mode but {why}; only a "
                    f"leading prefix of the trunk can run on its running statistics")
        if e > g:
            raise RuntimeError(
                f"CILRS fine-tuning: BatchNorm {groups[g][1][0][0]} is in eval mode but the "
                f"parameters of its group ({TRUNK_GROUPS[g]}) are trainable; frozen statistics "
                f"under trainable weights are not supported (freeze the parameters too)")
        if 0 < e < g:
            raise RuntimeError(
                f"CILRS fine-tuning: BatchNorm {groups[e][1][0][0]} is in train mode but "
                f"{groups[e - 1][1][0][0]} is in eval mode, inside the frozen prefix of {g} "
                f"group(s); put the whole frozen prefix in eval mode, or none of it")
        return e, g

    def freeze(self, upto):
        """Freeze the trunk up to and including group `upto` ("stem", "layer1" .. "layer4"):
        ``requires_grad_(False)`` on its parameters and ``.eval()`` on its modules -- exactly
        torch's idiom, nothing else.  Groups behind it are made trainable / put in the model's
        mode.  ``model.train()`` clears the eval flags again, as in torch: call ``freeze`` after it
        (``Trainer.train_step`` calls ``model.train()`` only when the model is in eval mode)."""
        if upto not in TRUNK_GROUPS:
            raise ValueError(f"freeze(upto): one of {TRUNK_GROUPS}, got {upto!r}")
        k = TRUNK_GROUPS.index(upto) + 1
        for gi, children in enumerate(_GROUP_CHILDREN):
            for ci in children:
                child = self.visual_encoder[ci]
                child.requires_grad_(gi >= k)
                child.train(self.training and gi >= k)
        return self

    def unfreeze(self):
        """Undo ``freeze``: every trunk parameter trainable, every trunk module in the model's mode."""
        for children in _GROUP_CHILDREN:
            for ci in children:
                child = self.visual_encoder[ci]
                child.requires_grad_(True)
                child.train(self.training)
        return self

    # -- engine plumbing ---------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        # .to()/.cuda()/.cpu() re-create parameter storage: the flat arena must be rebuilt
        self._engine = None
        self.__dict__.pop("_ft_lists", None)
        return super()._apply(fn, *a, **k)

    def engine(self) -> Engine:
        """The HIP engine bound to this module's parameters (built on first use)."""
        eng = self._engine
        if eng is None or not eng.is_attached():
            # architecture code of the C-ABI: trunk | num_commands << 8 (0 = the reference's 4)
            code = self.VARIANT | ((self.num_commands << 8) if self.num_commands != 4 else 0)
            eng = Engine(self, code)
            self._engine = eng
            _track(self)
        return eng

    # -- the reference's forward signature -----------------------------------------------------
    def forward(self, image, speed, command):
        eng = self.engine()
        seed = 0
        p = self.dropout if self.training else 0.0
        if p > 0.0:
            from .train import dropout_seed
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            self._dropout_calls += 1
            seed = dropout_seed(torch.initial_seed(), self._dropout_calls, rank)
        return eng.forward(image, speed, command, self.training, p, seed)


def _track(module):
    """In-place parameter writes made while the module stays in eval mode (frozen-BatchNorm
    fine-tuning with torch.optim, ...) must invalidate the engine's cached inference state.  One
    global optimizer post-step hook bumps the weights epoch of every live engine whose parameters
    the stepping optimizer owns."""
    import weakref
    if CILRS._live is None:
        CILRS._live = weakref.WeakSet()

        def _after_step(optimizer, *_a, **_k):
            owned = {id(p) for g in optimizer.param_groups for p in g["params"]}
            for m in list(CILRS._live):
                eng = m._engine
                if eng is not None and id(eng._first_param) in owned:
                    eng.weights_epoch += 1
        from torch.optim.optimizer import register_optimizer_step_post_hook
        register_optimizer_step_post_hook(_after_step)
    CILRS._live.add(module)


class CILRSResNet50(CILRS):
    """BASELINE.json configs[3]: the same CILRS heads on a ResNet-50 trunk (torchvision-style
    Bottleneck stacks [3,4,6,3], stride on the 3x3 convolution; 2048-d features, so the first
    Linear of every branch is 2176 wide and the speed predictor's 2048 wide).  The reference has
    no such model (model/autonomous_drive.py:365 is resnet34 only); state_dict keys follow the
    same re-wrapping (visual_encoder.{4..7}.{blk}.{conv1,bn1,conv2,bn2,conv3,bn3,downsample}).
    Trains in fp32 through the same HIP kernels as the reference network (train-mode forward,
    backward, Trainer); inference in fp32, or through Engine.run_forward_u8(half="bf16") with the
    trunk on the bf16 matrix pipe."""
    VARIANT = 1
    FEATURES = 2048

    def _trunk(self):
        return nn.Sequential(
            nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.MaxPool2d(3, 2, 1),
            _make_bottleneck_layer(64, 64, 3, 1), _make_bottleneck_layer(256, 128, 4, 2),
            _make_bottleneck_layer(512, 256, 6, 2), _make_bottleneck_layer(1024, 512, 3, 2),
            nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten())
