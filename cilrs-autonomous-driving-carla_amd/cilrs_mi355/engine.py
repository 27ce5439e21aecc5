"""Host side of the HIP engine: flat parameter arenas, per-shape plans, autograd bridge.

PyTorch is used here for device memory, streams and autograd plumbing only; every number is
produced by libcilrs_hip.so (see include/cilrs_hip.h).

Memory layout (all fp32, on one device):
  * ``params``   flat arena in ``nn.Module.parameters()`` order (cilrs_param_info); each
                 ``nn.Parameter.data`` is a VIEW into it.  Conv weights are stored OHWI and exposed
                 as logical-OIHW permuted views (= torch channels_last memory), so
                 ``state_dict()`` / ``load_state_dict()`` / any ``torch.optim`` work unchanged
                 (reference contract: model/autonomous_drive.py:496-497,
                 notebook/notebook.ipynb:533, 631-636).
  * ``grads``    same layout; backward writes it, Adam / clip / all-reduce read it.
  * ``bn``       running_mean / running_var arena + int64[36] num_batches_tracked.
  * workspace    one allocation per (batch, H, W) plan holding every saved activation.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L

import operator

_VERSION_OF = operator.attrgetter("_version")

SEG_NAMES = ("heads", "layer4", "layer3", "layer2", "layer1", "stem")


def _layout(variant=0):
    """(parameter layout, BatchNorm layout) of architecture `variant` (0: the reference's
    ResNet-34 network; 1: the ResNet-50 variant of BASELINE.json configs[3])."""
    lib = L.lib()
    params = []
    name = C.create_string_buffer(256)
    for i in range(lib.cilrs_variant_num_params(variant)):
        off, numel, ndim = L.sz(), L.sz(), L.i32()
        shape = (L.i32 * 4)()
        L.check(lib.cilrs_variant_param_info(variant, i, name, 256, C.byref(off), C.byref(numel),
                                             C.byref(ndim), shape))
        params.append((name.value.decode(), off.value, numel.value,
                       tuple(shape[k] for k in range(ndim.value))))
    bns = []
    for j in range(lib.cilrs_variant_num_bn(variant)):
        ch, rm, rv = L.i32(), L.sz(), L.sz()
        L.check(lib.cilrs_variant_bn_info(variant, j, name, 256, C.byref(ch), C.byref(rm),
                                          C.byref(rv)))
        bns.append((name.value.decode(), ch.value, rm.value, rv.value))
    return params, bns


def segment_ranges(variant=0):
    """[(begin, end)] float ranges of the gradient arena, in backward execution order."""
    lib = L.lib()
    out = []
    for s in range(6):
        b, e = L.sz(), L.sz()
        L.check(lib.cilrs_variant_segment_range(variant, s, C.byref(b), C.byref(e)))
        out.append((b.value, e.value))
    return out


def group_ranges(variant=0):
    """[(begin, end)] float ranges of the arena per parameter group, in arena (= parameters())
    order: stem, layer1, layer2, layer3, layer4, heads.  Contiguous; starts are 16-byte aligned."""
    segs = segment_ranges(variant)
    return [segs[5], segs[4], segs[3], segs[2], segs[1], segs[0]]


def _arena_view(arena, off, numel, shape):
    flat = arena[off:off + numel]
    if len(shape) == 4:                       # OHWI storage, logical OIHW
        o, i, h, w = shape
        return flat.view(o, h, w, i).permute(0, 3, 1, 2)
    return flat.view(shape)


PLAN_BF16_TRAIN = 1       # include/cilrs_hip.h CILRS_PLAN_BF16_TRAIN


class Plan:
    """cilrs_net for one (batch, H, W) + its workspace."""

    def __init__(self, device, batch, h, w, variant=0, flags=0):
        lib = L.lib()
        handle = L.vp()
        L.check(lib.cilrs_net_create_ex(variant, batch, h, w, flags, C.byref(handle)))
        self.flags = flags
        self.handle = handle
        self.batch, self.h, self.w = batch, h, w
        nbytes = lib.cilrs_net_workspace_bytes(handle)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
        assert self.workspace.data_ptr() % 256 == 0
        # int32[4] status words inside the workspace (word 0: a command outside 0..3 was seen by
        # a forward SINCE THE LAST check_status() -- the reference's torch.gather raises there,
        # autonomous_drive.py:397; kernels only ever set the words, so one read at the end of an
        # epoch covers every batch; word 1: a grid barrier of the persistent launch gave up)
        off = lib.cilrs_net_status_offset(handle)
        self.status = self.workspace[off:off + 16].view(torch.int32)
        self.status.zero_()
        self.generation = 0

    def __del__(self):
        try:
            if self.handle:
                L.lib().cilrs_net_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def take_status(self):
        """Synchronising read-and-clear of the status words: (bad_command, barrier_gave_up)."""
        dev = self.workspace.device
        torch.cuda.synchronize(dev)
        st = self.status.tolist()
        if st[0] != 0 or st[1] != 0:
            self.status.zero_()
            torch.cuda.synchronize(dev)
        return st[0] != 0, st[1] != 0

    def check_status(self):
        """Synchronising read of the status words of the last forward on this plan; raises what
        the reference's ``all_out.gather(0, idx)`` raises for an out-of-range command."""
        # forwards may have run on other streams than torch's current one (Predictor, inference
        # lanes): wait for the whole device before reading, and again after clearing, so that a
        # set racing the clear cannot be lost
        dev = self.workspace.device
        torch.cuda.synchronize(dev)
        st = self.status.tolist()
        if st[0] != 0 or st[1] != 0:
            self.status.zero_()           # the words are sticky: "since the last check"
            torch.cuda.synchronize(dev)
        if st[1] != 0:
            raise RuntimeError("CILRS persistent forward: a grid barrier gave up (another "
                               "persistent launch was holding the device); outputs are NaN")
        if st[0] != 0:
            raise RuntimeError("CILRS.forward: command index out of range (expected 0..num_commands-1); "
                               "torch.gather raises 'index out of bounds' here "
                               "(model/autonomous_drive.py:397-398)")

    # per-kernel hipEvent timing ------------------------------------------------------------
    def profile(self, on: bool):
        L.check(L.lib().cilrs_net_profile_enable(self.handle, 1 if on else 0))

    def profile_reset(self):
        L.check(L.lib().cilrs_net_profile_reset(self.handle))

    def ft_wino_convs(self) -> int:
        """Folded-epilogue Winograd launches of the plan's last fine-tuning forward."""
        return int(L.lib().cilrs_net_ft_wino_convs(self.handle))

    def wino_convs(self) -> int:
        """Convolutions of this plan's train step that run on the Winograd kernel (0: none)."""
        return int(L.lib().cilrs_net_wino_convs(self.handle))

    def profile_table(self):
        lib = L.lib()
        L.check(lib.cilrs_net_profile_collect(self.handle))
        rows = {}
        label = C.create_string_buffer(128)
        for i in range(lib.cilrs_net_profile_count(self.handle)):
            calls, ms, fl, by = C.c_longlong(), L.f64(), L.f64(), L.f64()
            L.check(lib.cilrs_net_profile_entry(self.handle, i, label, 128, C.byref(calls),
                                                C.byref(ms), C.byref(fl), C.byref(by)))
            rows[label.value.decode()] = dict(calls=calls.value, ms=ms.value, flops=fl.value,
                                              bytes=by.value)
        return rows


class Engine:
    def __init__(self, module, variant=0):
        lib = L.lib()                                    # raises if the extension is missing
        self.variant = variant
        named = list(module.named_parameters())
        if not named:
            raise RuntimeError("CILRS has no parameters")
        device = named[0][1].device
        if device.type != "cuda":
            raise RuntimeError(
                "CILRS.forward runs only on a ROCm device (model.to('cuda')): the MI355X HIP "
                "engine has no CPU fallback")
        self.device = device
        self.module = module
        self.params_layout, self.bn_layout = _layout(variant)
        names = [n for n, _ in named]
        want = [p[0] for p in self.params_layout]
        if names != want:
            raise RuntimeError("module parameter names differ from the engine layout")
        n_arena = lib.cilrs_variant_param_arena_floats(variant)
        self.n_arena = n_arena
        self.params = torch.zeros(n_arena, dtype=torch.float32, device=device)
        self.grads = torch.zeros(n_arena, dtype=torch.float32, device=device)
        self.bn = torch.zeros(lib.cilrs_variant_bn_arena_floats(variant), dtype=torch.float32,
                              device=device)
        self.nbt = torch.zeros(len(self.bn_layout), dtype=torch.int64, device=device)
        self.param_views, self.grad_views = [], []
        with torch.no_grad():
            for (name, p), (_, off, numel, shape) in zip(named, self.params_layout):
                if p.dtype != torch.float32 or tuple(p.shape) != shape:
                    raise RuntimeError(f"{name}: expected float32 {shape}, got {p.dtype} "
                                       f"{tuple(p.shape)}")
                v = _arena_view(self.params, off, numel, shape)
                v.copy_(p.data)
                old_grad = p.grad
                p.data = v
                g = _arena_view(self.grads, off, numel, shape)
                if old_grad is not None:
                    g.copy_(old_grad)
                    p.grad = g
                self.param_views.append(v)
                self.grad_views.append(g)
            mods = dict(module.named_modules())
            for j, (prefix, ch, rm, rv) in enumerate(self.bn_layout):
                bnm = mods[prefix]
                for attr, off in (("running_mean", rm), ("running_var", rv)):
                    v = self.bn[off:off + ch]
                    v.copy_(getattr(bnm, attr))
                    setattr(bnm, attr, v)          # registered buffer keeps its name
                v = self.nbt[j]
                v.copy_(bnm.num_batches_tracked)
                bnm.num_batches_tracked = v
        self._first_param = named[0][1]
        self._last_param = named[-1][1]
        self.plans = {}
        self.bufs = {}
        self.last_plan = None
        self._followup_bufs = {}          # (follow-up, owner, shape...) -> scratch + pinned outputs
        # "fp32" (the reference's arithmetic) or "bf16": train-mode trunk convolutions on the bf16
        # matrix pipe (include/cilrs_hip.h CILRS_PLAN_BF16_TRAIN); set through
        # Trainer(..., precision=) or directly before the first train-mode forward
        self.train_precision = "fp32"
        self._scratch_grads = None        # second gradient arena (autograd accumulation only)
        # False: loss.backward() hands autograd CLONES of the gradient arena (torch semantics: they
        # stay valid whatever runs next).  True: views of the arena, valid until the next backward.
        self.zero_copy_grads = False
        self.weights_epoch = 1            # bumped by every kernel-side write to params / BN buffers
        # torch-visible in-place edits (`with torch.no_grad(): p.mul_(2)`) bump the tensors' version
        # counters: the eval-mode `model(...)` call -- the reference's own inference call -- polls
        # them (poll_versions), the latency paths rely on the weights_changed() contract instead
        self._versioned = tuple(p for _n, p in named) + tuple(
            b for m in module.modules() if isinstance(m, torch.nn.BatchNorm2d)
            for b in (m.running_mean, m.running_var))
        self._version_sum = sum(map(_VERSION_OF, self._versioned))
        # fine-tuning: arena range per parameter group, and the key under which a plan caches the
        # weight-derived state of a frozen prefix (a new value whenever the cut changes or
        # anything but a fine-tuning step of the same cut moved the weights epoch)
        self.group_ranges = group_ranges(variant)
        self._ft_epoch, self._ft_cut, self._ft_expect = 0, 0, -1

    # ------------------------------------------------------------------------------------------
    def is_attached(self) -> bool:
        a, b = self._first_param, self._last_param
        return (a.data_ptr() == self.params.data_ptr() and a.device == self.device
                and b.device == self.device)

    def plan(self, batch, h, w, lane=0) -> Plan:
        """The cilrs_net + workspace for one (batch, H, W).  `lane` > 0 gives further,
        independent plans of the same geometry: concurrent inference streams (each on its own
        HIP stream) must not share a workspace."""
        flags = PLAN_BF16_TRAIN if self.train_precision == "bf16" else 0
        key = (batch, h, w) if lane == 0 else (batch, h, w, lane)
        if flags:
            key = key + ("flags", flags)
        pl = self.plans.get(key)
        if pl is None:
            pl = Plan(self.device, batch, h, w, self.variant, flags)
            self.plans[key] = pl
            pl.bufs = L.Buffers(self.params.data_ptr(), self.grads.data_ptr(),
                                self.bn.data_ptr(), self.nbt.data_ptr(),
                                pl.workspace.data_ptr())
            self.bufs[key] = pl.bufs
        return pl

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def weights_key(self) -> int:
        """Non-zero value that changes whenever the parameters or BatchNorm buffers may have
        changed.  O(1) -- it sits on the single-frame latency path.  `weights_epoch` is bumped by
        every kernel-side write (train-mode forward, fused Adam), by load_state_dict and by every
        train()/eval() switch of the module (model.py hooks); code that writes parameters in
        place by other means while the module stays in eval mode calls CILRS.weights_changed()."""
        return (self.weights_epoch * 0xD6E8FEB86659FD93) & 0xFFFFFFFFFFFFFFFF or 1

    def poll_versions(self) -> bool:
        """Bump the weights epoch if any parameter / BatchNorm buffer was modified in place through
        torch since the last poll (sum of the tensors' `_version` counters: ~20 us for the 250
        tensors, so only the eval-mode `model(...)` call does it on every use; Predictor and
        run_forward_u8 -- the latency paths -- rely on CILRS.weights_changed()).  Edits that torch
        cannot see (`p.data`, raw pointers) always need weights_changed()."""
        v = sum(map(_VERSION_OF, self._versioned))
        if v == self._version_sum:
            return False
        self._version_sum = v
        self.weights_epoch += 1
        return True

    def _announce_weights(self, pl):
        L.check(L.lib().cilrs_net_set_weights_key(pl.handle, self.weights_key()))

    # ------------------------------------------------------------------------------------------
    def _check_inputs(self, image, speed, command):
        if image.dim() != 4 or image.size(1) != 3:
            raise RuntimeError(f"image must be [B,3,H,W], got {tuple(image.shape)}")
        b = image.size(0)
        if image.dtype != torch.float32 or speed.dtype != torch.float32:
            raise RuntimeError("image and speed must be float32")
        if command.dtype != torch.int64:
            raise RuntimeError("command must be int64 (torch.long), as torch.gather requires")
        if tuple(speed.shape) != (b,) or tuple(command.shape) != (b,):
            raise RuntimeError("speed and command must have shape [B]")
        for t in (image, speed, command):
            if t.device != self.device:
                raise RuntimeError(f"input on {t.device}, model on {self.device}")
        return b

    def run_forward(self, image, speed, command, train, dropout_p, seed):
        """Enqueue the forward; returns (controls, pred_speed, plan)."""
        b = self._check_inputs(image, speed, command)
        pl = self.plan(b, image.size(2), image.size(3))
        speed = speed.contiguous()
        command = command.contiguous()
        controls = torch.empty(b, 3, dtype=torch.float32, device=self.device)
        pred_speed = torch.empty(b, dtype=torch.float32, device=self.device)
        sn, sc, sh, sw = image.stride()
        if train:
            self.weights_epoch += 1           # BN running statistics are about to move
        else:
            self.poll_versions()
        self._announce_weights(pl)
        L.check(L.lib().cilrs_net_forward(
            pl.handle, C.byref(pl.bufs), L.ptr(image), sn, sc, sh, sw,
            L.ptr(speed), L.ptr(command), 1 if train else 0, float(dropout_p), int(seed),
            L.ptr(controls), L.ptr(pred_speed), self._stream()))
        if train:
            pl.generation += 1
        self.last_plan = pl
        return controls, pred_speed, pl

    def run_forward_bn_stats(self, image, table):
        """Enqueue the train-mode trunk on `image` with every BatchNorm's batch statistics added to
        the float64 device `table` (cilrs_net_forward_bn_stats; bn_estimate.py): no heads, the
        running buffers and the parameters untouched, no host synchronisation.  Returns the plan."""
        if image.dim() != 4 or image.size(1) != 3:
            raise RuntimeError(f"image must be [B,3,H,W], got {tuple(image.shape)}")
        if image.dtype != torch.float32:
            raise RuntimeError("image must be float32")
        if image.device != self.device or table.device != self.device:
            raise RuntimeError(f"image on {image.device}, table on {table.device}, model on "
                               f"{self.device}")
        n = L.lib().cilrs_variant_bn_stats_doubles(self.variant)
        if table.dtype != torch.float64 or table.numel() != n or not table.is_contiguous():
            raise RuntimeError(f"table must be a contiguous float64 tensor of {n} entries")
        if self.train_precision != "fp32":
            raise RuntimeError("BatchNorm re-estimation: fp32 plans only")
        pl = self.plan(image.size(0), image.size(2), image.size(3))
        sn, sc, sh, sw = image.stride()
        # the plan's per-layer scale / shift tables are about to hold batch statistics: what any
        # plan cached from them (eval state, a fine-tuning prefix) is rebuilt on its next use
        self.weights_epoch += 1
        self._announce_weights(pl)
        L.check(L.lib().cilrs_net_forward_bn_stats(
            pl.handle, C.byref(pl.bufs), L.ptr(image), sn, sc, sh, sw, L.ptr(table),
            self._stream()))
        pl.generation += 1                    # the saved activations of earlier graphs are gone
        self.last_plan = pl
        return pl

    def trainable_begin(self, frozen_groups) -> int:
        """First arena float of the trainable range behind `frozen_groups` frozen trunk groups."""
        return self.group_ranges[frozen_groups][0]

    def check_freeze(self, e, g, image=None):
        """What no fine-tuning step can serve (raised before any launch)."""
        if g and self.train_precision == "bf16":
            raise RuntimeError("CILRS fine-tuning: the bf16 training plan cannot freeze trunk "
                               "groups (fp32 training only)")
        if g and image is not None and image.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("CILRS fine-tuning: image.requires_grad is set but the trunk is "
                               f"frozen up to {SEG_NAMES[6 - g]}; input gradients through a frozen "
                               "prefix are not supported")

    def wrote_trainable(self, e):
        """A kernel updated parameters behind an eval-mode prefix of `e` groups only (the ranged
        Adam of a fine-tuning step): everything cached for inference is stale, the prefix's own
        state is not."""
        keep = e > 0 and self._ft_cut == e and self._ft_expect == self.weights_epoch
        self.weights_epoch += 1
        if keep:
            self._ft_expect = self.weights_epoch

    def snapshot_bn(self, bn, nbt):
        """Copy the running statistics and num_batches_tracked into `bn` / `nbt` (same shapes)."""
        with torch.no_grad():
            bn.copy_(self.bn)
            nbt.copy_(self.nbt)

    def put_back_bn(self, bn, nbt):
        """Inverse of snapshot_bn, bit for bit.  The statistics go back through the library's copy
        kernel, not torch's copy_: that would bump the version counters poll_versions watches, and
        with them the key of a frozen prefix's cached state, on every step."""
        L.check(L.lib().cilrs_sam_restore(L.ptr(self.bn), L.ptr(bn), self.bn.numel(),
                                          self._stream()))
        with torch.no_grad():
            self.nbt.copy_(nbt)                   # (not among the polled tensors)

    def run_forward_ft(self, image, speed, command, e, g, dropout_p, seed):
        """Train-mode forward with the first `g` trunk groups taking no gradient and the first
        `e` (0 or g) of them in eval mode (cilrs_net_forward_ft); (0, 0) is run_forward."""
        if e == 0 and g == 0:
            return self.run_forward(image, speed, command, True, dropout_p, seed)
        self.check_freeze(e, g)
        b = self._check_inputs(image, speed, command)
        pl = self.plan(b, image.size(2), image.size(3))
        speed = speed.contiguous()
        command = command.contiguous()
        controls = torch.empty(b, 3, dtype=torch.float32, device=self.device)
        pred_speed = torch.empty(b, dtype=torch.float32, device=self.device)
        sn, sc, sh, sw = image.stride()
        key = 0
        if e > 0:
            self.poll_versions()              # torch-visible edits of the frozen prefix
            if self._ft_cut != e or self._ft_expect != self.weights_epoch:
                self._ft_epoch += 1
            self._ft_cut = e
            key = (self._ft_epoch * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF or 1
        self.weights_epoch += 1               # BN running statistics behind the prefix move
        self._ft_expect = self.weights_epoch if e > 0 else -1      # (e == 0: the prefix's move too)
        self._announce_weights(pl)
        L.check(L.lib().cilrs_net_forward_ft(
            pl.handle, C.byref(pl.bufs), L.ptr(image), sn, sc, sh, sw,
            L.ptr(speed), L.ptr(command), int(e), int(g), key, float(dropout_p), int(seed),
            L.ptr(controls), L.ptr(pred_speed), self._stream()))
        pl.generation += 1
        self.last_plan = pl
        return controls, pred_speed, pl

    def run_forward_frozen(self, image, speed, command):
        """model.eval() forward that keeps its graph (BatchNorm on the running statistics, no
        dropout, running buffers untouched): the forward of an eval-mode autograd graph.
        Returns (controls, pred_speed, plan)."""
        b = self._check_inputs(image, speed, command)
        pl = self.plan(b, image.size(2), image.size(3))
        speed = speed.contiguous()
        command = command.contiguous()
        controls = torch.empty(b, 3, dtype=torch.float32, device=self.device)
        pred_speed = torch.empty(b, dtype=torch.float32, device=self.device)
        sn, sc, sh, sw = image.stride()
        self.poll_versions()
        self._announce_weights(pl)
        L.check(L.lib().cilrs_net_forward_frozen(
            pl.handle, C.byref(pl.bufs), L.ptr(image), sn, sc, sh, sw,
            L.ptr(speed), L.ptr(command), L.ptr(controls), L.ptr(pred_speed), self._stream()))
        pl.generation += 1                    # the saved activations of earlier graphs are gone
        self.last_plan = pl
        return controls, pred_speed, pl

    def run_forward_frozen_u8(self, frames_u8, speed, command, height=None, width=None, out=None):
        """run_forward_frozen fed with uint8 frames (device tensors): [B,H,W,3] at the network
        resolution (height / width None), or raw camera frames [B,Hs,Ws,3|4] resized on the device
        to (height, width) like run_forward_camera.  Returns (controls, pred_speed, plan)."""
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.size(3) not in (3, 4):
            raise RuntimeError("frames must be uint8 [B,H,W,3] (camera frames: 3 or 4 bytes per pixel)")
        camera = height is not None
        if not camera and frames_u8.size(3) != 3:
            raise RuntimeError("frames at the network resolution must be uint8 [B,H,W,3]")
        b = frames_u8.size(0)
        pl = self.plan(b, height, width) if camera else self.plan(b, frames_u8.size(1),
                                                                  frames_u8.size(2))
        frames_u8 = frames_u8.contiguous()
        if out is None:
            controls = torch.empty(b, 3, dtype=torch.float32, device=self.device)
            pred_speed = torch.empty(b, dtype=torch.float32, device=self.device)
        else:
            controls, pred_speed = out
        self._announce_weights(pl)
        lib = L.lib()
        if camera:
            hs, ws, px = frames_u8.size(1), frames_u8.size(2), frames_u8.size(3)
            L.check(lib.cilrs_net_forward_frozen_camera(
                pl.handle, C.byref(pl.bufs), L.ptr(frames_u8), hs, ws, px, ws * px, hs * ws * px,
                L.ptr(speed.contiguous()), L.ptr(command.contiguous()), L.ptr(controls),
                L.ptr(pred_speed), self._stream()))
        else:
            L.check(lib.cilrs_net_forward_frozen_u8(
                pl.handle, C.byref(pl.bufs), L.ptr(frames_u8), L.ptr(speed.contiguous()),
                L.ptr(command.contiguous()), L.ptr(controls), L.ptr(pred_speed), self._stream()))
        pl.generation += 1                    # the saved activations of earlier graphs are gone
        self.last_plan = pl
        return controls, pred_speed, pl

    def run_saliency_map(self, dimage, chan_scale3=None, heat=None, heat_u8=None, peak=None):
        """cilrs_saliency_map over an image gradient [B,3,H,W] (any strides): fills and returns
        (heat float32 [B,H,W], peak float32 [B]); heat_u8 (uint8 [B,H,W]) is filled when given."""
        if dimage.dtype != torch.float32 or dimage.dim() != 4 or dimage.size(1) != 3:
            raise RuntimeError("dimage must be float32 [B,3,H,W]")
        b, _, h, w = dimage.shape
        if heat is None:
            heat = torch.empty(b, h, w, dtype=torch.float32, device=self.device)
        if peak is None:
            peak = torch.empty(b, dtype=torch.float32, device=self.device)
        for t, dt, shape in ((heat, torch.float32, (b, h, w)), (peak, torch.float32, (b,)),
                             (heat_u8, torch.uint8, (b, h, w))):
            if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()
                                  or t.device != dimage.device):
                raise RuntimeError(f"saliency map outputs must be contiguous {dt} {shape} on "
                                   f"{dimage.device}")
        scale = None
        if chan_scale3 is not None:
            scale = (C.c_float * 3)(*[float(v) for v in chan_scale3])
        L.check(L.lib().cilrs_saliency_map(
            L.ptr(dimage), *dimage.stride(), b, h, w, scale, L.ptr(heat), L.ptr(heat_u8),
            L.ptr(peak), self._stream()))
        return heat, peak

    # ---- SmoothGrad / integrated gradients (csrc/attribution.hip) ------------------------------
    def _check_attr_frames(self, frames_u8, baseline_u8):
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.size(3) != 3 or \
                not frames_u8.is_contiguous() or frames_u8.device != self.device:
            raise RuntimeError(f"frames must be contiguous uint8 [B,H,W,3] on {self.device}")
        if baseline_u8 is not None and (baseline_u8.dtype != torch.uint8 or
                                        baseline_u8.shape != frames_u8.shape or
                                        not baseline_u8.is_contiguous() or
                                        baseline_u8.device != self.device):
            raise RuntimeError(f"baseline must be contiguous uint8 {tuple(frames_u8.shape)} on "
                               f"{self.device}")
        return frames_u8.size(0), frames_u8.size(1), frames_u8.size(2)

    def run_attr_samples(self, frames_u8, baseline_u8, mode, samples, s_begin, s_count, sigma255,
                         seed, out=None):
        """cilrs_attr_samples: samples [s_begin, s_begin + s_count) of `samples` per frame of
        uint8 [B,H,W,3] -> float32 NCHW [B*s_count,3,H,W] (frame-major); fills and returns `out`."""
        b, h, w = self._check_attr_frames(frames_u8, baseline_u8)
        if out is None:
            out = torch.empty(b * s_count, 3, h, w, dtype=torch.float32, device=self.device)
        elif (out.dtype != torch.float32 or tuple(out.shape) != (b * s_count, 3, h, w) or
              not out.is_contiguous() or out.device != self.device):
            raise RuntimeError(f"samples must be contiguous float32 [{b * s_count},3,{h},{w}] on "
                               f"{self.device}")
        L.check(L.lib().cilrs_attr_samples(
            L.ptr(frames_u8), L.ptr(baseline_u8), b, h, w, int(mode), int(samples), int(s_begin),
            int(s_count), float(sigma255), int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(out),
            self._stream()))
        return out

    def run_attr_accumulate(self, dimage, acc, s_count, first):
        """cilrs_attr_accumulate: acc [B,3,H,W] (+)= the gradients [B*s_count,3,H,W] (any
        strides) of each frame's samples in sample order; `first` starts the sum at zero."""
        if acc.dtype != torch.float32 or acc.dim() != 4 or acc.size(1) != 3 or \
                not acc.is_contiguous() or acc.device != self.device:
            raise RuntimeError(f"acc must be contiguous float32 [B,3,H,W] on {self.device}")
        b, _, h, w = acc.shape
        if dimage.dtype != torch.float32 or tuple(dimage.shape) != (b * s_count, 3, h, w) or \
                dimage.device != self.device:
            raise RuntimeError(f"dimage must be float32 [{b * s_count},3,{h},{w}] on {self.device}")
        L.check(L.lib().cilrs_attr_accumulate(
            L.ptr(dimage), *dimage.stride(), b, int(s_count), h, w, 1 if first else 0, L.ptr(acc),
            self._stream()))
        return acc

    def run_attr_finalize(self, acc, frames_u8, baseline_u8, mode, samples, chan_scale3=None,
                          attr=None, signed_map=None, total=None):
        """cilrs_attr_finalize over the gradient sum acc [B,3,H,W]: fills and returns attr
        float32 [B,3,H,W]; signed_map [B,H,W] and total [B] are filled when given."""
        if acc.dtype != torch.float32 or acc.dim() != 4 or acc.size(1) != 3 or \
                not acc.is_contiguous() or acc.device != self.device:
            raise RuntimeError(f"acc must be contiguous float32 [B,3,H,W] on {self.device}")
        b, _, h, w = acc.shape
        if frames_u8 is not None and self._check_attr_frames(frames_u8, baseline_u8) != (b, h, w):
            raise RuntimeError(f"frames must be uint8 [{b},{h},{w},3]")
        if attr is None:
            attr = torch.empty(b, 3, h, w, dtype=torch.float32, device=self.device)
        for t, shape in ((attr, (b, 3, h, w)), (signed_map, (b, h, w)), (total, (b,))):
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or
                                  not t.is_contiguous() or t.device != self.device):
                raise RuntimeError(f"attribution outputs must be contiguous float32 {shape} on "
                                   f"{self.device}")
        scale = None
        if chan_scale3 is not None:
            scale = (C.c_float * 3)(*[float(v) for v in chan_scale3])
        L.check(L.lib().cilrs_attr_finalize(
            L.ptr(acc), L.ptr(frames_u8), L.ptr(baseline_u8), b, h, w, int(mode), int(samples),
            scale, L.ptr(attr), L.ptr(signed_map), L.ptr(total), self._stream()))
        return attr

    # ---- FGSM / PGD (csrc/adversarial.hip) ------------------------------------------------------
    def _check_adv_image(self, t, name, shape=None):
        if t.dtype != torch.float32 or t.dim() != 4 or t.size(1) != 3 or t.device != self.device:
            raise RuntimeError(f"{name} must be float32 [B,3,H,W] on {self.device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"{name} must be float32 {tuple(shape)}, got {tuple(t.shape)}")
        return t.size(0), t.size(2), t.size(3)

    def _check_adv_rows(self, t, name, dtype, shape):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
                              or t.device != self.device):
            raise RuntimeError(f"{name} must be contiguous {dtype} {shape} on {self.device}")

    @staticmethod
    def _adv_floats(values, n):
        return None if values is None else (C.c_float * n)(*[float(v) for v in values])

    def run_adv_start(self, x, eps255, chan_scale3, seed, x_adv, range6=None):
        """cilrs_adv_start: x_adv = x + e_c * (2u - 1) clamped to the eps ball (and range6), the
        draw keyed on `seed` and the logical element index; eps255 = 0 is a copy.  x and x_adv
        float32 [B,3,H,W] with any strides; fills and returns x_adv."""
        b, h, w = self._check_adv_image(x, "x")
        self._check_adv_image(x_adv, "x_adv", x.shape)
        L.check(L.lib().cilrs_adv_start(
            L.ptr(x), *x.stride(), b, h, w, float(eps255), self._adv_floats(chan_scale3, 3),
            int(seed) & 0xFFFFFFFFFFFFFFFF, self._adv_floats(range6, 6), L.ptr(x_adv),
            *x_adv.stride(), self._stream()))
        return x_adv

    def run_adv_step(self, x, x_adv, g, alpha255, eps255, chan_scale3, row_dir=None, improved=None,
                     best=None, range6=None):
        """cilrs_adv_step: where improved[b], best = x_adv; then x_adv = clamp(x_adv + a_c *
        row_dir[b] * sign(g)) in place.  x and x_adv must share their strides; g and best have
        their own.  alpha255 = 0 performs the copy alone (g may then be None)."""
        b, h, w = self._check_adv_image(x, "x")
        self._check_adv_image(x_adv, "x_adv", x.shape)
        if x.stride() != x_adv.stride():
            raise RuntimeError(f"x and x_adv must have the same strides, got {x.stride()} and "
                               f"{x_adv.stride()}")
        if g is not None:
            self._check_adv_image(g, "g", x.shape)
        if best is not None:
            self._check_adv_image(best, "best", x.shape)
        self._check_adv_rows(row_dir, "row_dir", torch.float32, (b,))
        self._check_adv_rows(improved, "improved", torch.int32, (b,))
        zero = (0, 0, 0, 0)
        L.check(L.lib().cilrs_adv_step(
            L.ptr(x), L.ptr(x_adv), *x.stride(), L.ptr(g), *(g.stride() if g is not None else zero),
            b, h, w, float(alpha255), float(eps255), self._adv_floats(chan_scale3, 3),
            L.ptr(row_dir), L.ptr(improved), L.ptr(best),
            *(best.stride() if best is not None else zero), self._adv_floats(range6, 6),
            self._stream()))
        return x_adv

    def run_adv_direction(self, controls, pred_speed, ref_controls, ref_speed, w4, first, dev,
                          best_dev, row_dir, improved):
        """cilrs_adv_direction: dev = w . (outputs - ref) per frame, row_dir = its sign (+1 at 0),
        improved = first or |dev| > |best_dev| (best_dev updated there)."""
        b = controls.size(0)
        for t, name, shape in ((controls, "controls", (b, 3)), (ref_controls, "ref_controls", (b, 3)),
                               (pred_speed, "pred_speed", (b,)), (ref_speed, "ref_speed", (b,)),
                               (dev, "dev", (b,)), (best_dev, "best_dev", (b,)),
                               (row_dir, "row_dir", (b,))):
            if t is None:
                raise RuntimeError(f"{name} must be a tensor")
            self._check_adv_rows(t, name, torch.float32, shape)
        if improved is None:
            raise RuntimeError("improved must be a tensor")
        self._check_adv_rows(improved, "improved", torch.int32, (b,))
        L.check(L.lib().cilrs_adv_direction(
            L.ptr(controls), L.ptr(pred_speed), L.ptr(ref_controls), L.ptr(ref_speed),
            self._adv_floats(w4, 4), b, 1 if first else 0, L.ptr(dev), L.ptr(best_dev),
            L.ptr(row_dir), L.ptr(improved), self._stream()))

    def run_adv_quantize(self, x_adv, frames_u8=None, out_u8=None, linf=None):
        """cilrs_adv_quantize: x_adv float32 [B,3,H,W] (any strides) -> uint8 [B,H,W,3] camera
        frames; linf (int32 [B], with the clean frames_u8) = max |q - frame| per frame.  Fills and
        returns out_u8."""
        b, h, w = self._check_adv_image(x_adv, "x_adv")
        if out_u8 is None:
            out_u8 = torch.empty(b, h, w, 3, dtype=torch.uint8, device=self.device)
        self._check_adv_rows(out_u8, "out_u8", torch.uint8, (b, h, w, 3))
        self._check_adv_rows(frames_u8, "frames_u8", torch.uint8, (b, h, w, 3))
        self._check_adv_rows(linf, "linf", torch.int32, (b,))
        L.check(L.lib().cilrs_adv_quantize(
            L.ptr(x_adv), *x_adv.stride(), L.ptr(frames_u8), b, h, w, L.ptr(out_u8), L.ptr(linf),
            self._stream()))
        return out_u8

    def check_status(self):
        """Raise if the last forward saw an out-of-range command (one device->host read)."""
        if self.last_plan is not None:
            self.last_plan.check_status()

    def run_forward_u8(self, frames_u8, speed, command, out=None, graph=False, half=False,
                       lane=0, persistent=False):
        """uint8 RGB HWC frames [B,H,W,3] -> eval forward with fused preprocessing.  With
        graph=True the launch sequence is replayed from a cached hipGraph (all tensors must keep
        their addresses; the current stream must not be the default stream).  half=True / "f16"
        runs the trunk in fp16, half="bf16" in bf16 (BatchNorm folded into 16-bit weights, fp32
        accumulation): batched serving.  Calls issued on different HIP streams at the same time
        must use different `lane`s (one workspace each).  persistent=True (one frame, fp32, the
        reference network): the whole forward is ONE launch whose workgroups stay resident and
        meet at in-launch grid barriers (csrc/infer_b1.hip) -- the control-loop path."""
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.size(3) != 3:
            raise RuntimeError("frames must be uint8 [B,H,W,3]")
        b = frames_u8.size(0)
        pl = self.plan(b, frames_u8.size(1), frames_u8.size(2), lane)
        frames_u8 = frames_u8.contiguous()
        if out is None:
            controls = torch.empty(b, 3, dtype=torch.float32, device=self.device)
            pred_speed = torch.empty(b, dtype=torch.float32, device=self.device)
        else:
            controls, pred_speed = out
        lib = L.lib()
        if persistent:
            if half or b != 1 or self.variant != 0:
                raise RuntimeError("persistent=True serves one fp32 frame of the reference network")
            fn = lib.cilrs_net_forward_u8_b1
        elif half == "bf16":
            fn = lib.cilrs_net_forward_u8_bf16_graph if graph else lib.cilrs_net_forward_u8_bf16
        elif half:
            fn = lib.cilrs_net_forward_u8_f16_graph if graph else lib.cilrs_net_forward_u8_f16
        else:
            fn = lib.cilrs_net_forward_u8_graph if graph else lib.cilrs_net_forward_u8
        self._announce_weights(pl)
        L.check(fn(pl.handle, C.byref(pl.bufs), L.ptr(frames_u8),
                   L.ptr(speed.contiguous()), L.ptr(command.contiguous()), L.ptr(controls),
                   L.ptr(pred_speed), self._stream()))
        self.last_plan = pl
        return controls, pred_speed

    MC_MAX_SAMPLES, MC_MAX_ROWS = 4096, 65536

    MC_CACHE_ENTRIES = 8

    def _followup_plan(self, who):
        """The plan a tick follow-up runs on: the last forward's."""
        if self.last_plan is None:
            raise RuntimeError(f"{who}: no forward yet")
        return self.last_plan

    def _followup_buffers(self, name, owner, shape, make, usable=None):
        """The device scratch and pinned host outputs of follow-up `name` for (owner, shape...),
        built by make() on a miss or where usable(bufs) says the cached ones no longer do.  Each
        follow-up keeps its MC_CACHE_ENTRIES most recently used entries: callers that may run at
        the same time on different streams (two Predictors on one model) pass themselves as
        `owner` and so never share a buffer."""
        cache, key = self._followup_bufs, (name, id(owner) if owner is not None else None) + shape
        bufs = cache.pop(key, None)
        if bufs is None or (usable is not None and not usable(bufs)):
            mine = [k for k in cache if k[0] == name]        # least recently used first
            for k in mine[:-(self.MC_CACHE_ENTRIES - 1)]:    # room for the new one
                del cache[k]
            bufs = make()
        cache[key] = bufs                                # (re-inserted: most recently used last)
        return bufs

    def run_heads_mc(self, speed, command, samples, p, seed=0, return_samples=False, owner=None):
        """Monte-Carlo dropout through the heads (include/cilrs_hip.h, cilrs_net_heads_mc) on the
        features the last eval-mode forward left in its plan: enqueues the launches on the current
        stream and returns (mean [B,4], std [B,4], samples [B,S,4] or None) as views of a PINNED
        host buffer that the kernels write -- valid after the stream is synchronised and until the
        next call with the same (B, S).  speed / command: the tensors the forward was given
        (device or pinned host).  Scratch and outputs are cached per (owner, B, S)
        (_followup_buffers)."""
        pl = self._followup_plan("run_heads_mc")
        samples, p, b = int(samples), float(p), pl.batch
        if not 1 <= samples <= self.MC_MAX_SAMPLES:
            raise ValueError(f"samples must be in 1..{self.MC_MAX_SAMPLES}")
        if b * samples > self.MC_MAX_ROWS:
            raise ValueError(f"batch * samples must not exceed {self.MC_MAX_ROWS}")
        if not 0.0 <= p < 1.0:                       # (NaN fails both comparisons)
            raise ValueError("dropout probability must be in [0, 1)")

        def make():
            n = L.lib().cilrs_heads_mc_scratch_floats(self.variant, b, samples)
            scratch = torch.empty(n, dtype=torch.float32, device=self.device)
            host = torch.zeros(b * 8 + b * samples * 4, dtype=torch.float32).pin_memory()
            return (scratch, host, host[:b * 4].view(b, 4), host[b * 4:b * 8].view(b, 4),
                    host[b * 8:].view(b, samples, 4))
        scratch, _host, mean, std, smp = self._followup_buffers("mc", owner, (b, samples), make)
        L.check(L.lib().cilrs_net_heads_mc(
            pl.handle, C.byref(pl.bufs), L.ptr(speed), L.ptr(command), samples, p,
            int(seed) & 0xFFFFFFFFFFFFFFFF, L.ptr(mean), L.ptr(std),
            L.ptr(smp) if return_samples else None, L.ptr(scratch), scratch.numel(),
            self._stream()))
        return mean, std, (smp if return_samples else None)

    # ---- Grad-CAM (csrc/gradcam.hip) ---------------------------------------------------------------
    GRADCAM_CHANNELS = (64, 128, 256, 512, 1024, 2048)

    @staticmethod
    def _gradcam_weights(weights4):
        w = [float(v) for v in weights4]
        if len(w) != 4 or not all(math.isfinite(v) for v in w):
            raise ValueError("four finite output weights expected")
        return (C.c_float * 4)(*w)

    def run_heads_input_grad(self, speed, command, weights4, pooled=None, featmap=None, g=None,
                             out4=None, status=None):
        """cilrs_heads_input_grad on this engine's weights: d (w . outputs) / d pooled features of
        the eval-mode heads, float32 [B, F].  Features: `pooled` [B, ld >= F] (features first) or
        `featmap` [B, HW, F], which the kernel pools.  Returns (g, out4 [B, 4] raw outputs)."""
        if (pooled is None) == (featmap is None):
            raise ValueError("exactly one of pooled and featmap must be given")
        src = pooled if pooled is not None else featmap
        feat = L.lib().cilrs_variant_feature_width(self.variant)
        want = 2 if pooled is not None else 3
        if src.dtype != torch.float32 or src.dim() != want or not src.is_contiguous() or \
                src.size(-1) < feat or (featmap is not None and src.size(-1) != feat):
            raise RuntimeError(f"features must be contiguous float32 [B,ld>={feat}] or [B,HW,{feat}]")
        b = src.size(0)
        if tuple(speed.shape) != (b,) or tuple(command.shape) != (b,):
            raise RuntimeError(f"{b} speeds and commands expected")
        w = self._gradcam_weights(weights4)
        if g is None:
            g = torch.empty(b, feat, dtype=torch.float32, device=self.device)
        if out4 is None:
            out4 = torch.empty(b, 4, dtype=torch.float32, device=self.device)
        L.check(L.lib().cilrs_heads_input_grad(
            self.variant, L.ptr(self.params), L.ptr(pooled), src.size(1) if pooled is not None else 0,
            L.ptr(featmap), src.size(1) if featmap is not None else 0, L.ptr(speed.contiguous()),
            L.ptr(command.contiguous()), w, b, L.ptr(g), L.ptr(out4), L.ptr(status), self._stream()))
        return g, out4

    def run_gradcam_map(self, act, height, width, dact=None, g=None, cam=None, peak=None, heat=None,
                        heat_u8=None):
        """cilrs_gradcam_map: act float32 [B,h,w,C] (NHWC) with its gradient `dact` (same shape) or
        the pooled gradient `g` [B,C] -> (cam [B,h,w], peak [B], heat [B,height,width]); heat_u8
        (uint8 [B,height,width]) is filled when given."""
        if (dact is None) == (g is None):
            raise ValueError("exactly one of dact and g must be given")
        if act.dtype != torch.float32 or act.dim() != 4 or not act.is_contiguous():
            raise RuntimeError("act must be contiguous float32 [B,h,w,C]")
        b, h, w, c = act.shape
        other, shape = (dact, (b, h, w, c)) if dact is not None else (g, (b, c))
        if other.dtype != torch.float32 or tuple(other.shape) != shape or not other.is_contiguous():
            raise RuntimeError(f"the gradient must be contiguous float32 {shape}")
        if cam is None:
            cam = torch.empty(b, h, w, dtype=torch.float32, device=self.device)
        if peak is None:
            peak = torch.empty(b, dtype=torch.float32, device=self.device)
        if heat is None:
            heat = torch.empty(b, height, width, dtype=torch.float32, device=self.device)
        L.check(L.lib().cilrs_gradcam_map(
            L.ptr(act), L.ptr(dact), L.ptr(g), b, h, w, c, int(height), int(width), L.ptr(cam),
            L.ptr(peak), L.ptr(heat), L.ptr(heat_u8), self._stream()))
        return cam, peak, heat

    def run_gradcam(self, speed, command, weights4, layer=4, want_u8=False, owner=None):
        """cilrs_net_gradcam on what the last forward left in its plan (layer 4: any fp32 eval-mode
        forward; layers 1..3: run_forward_frozen* followed by run_backward over segments
        (0, 5 - layer)).  Enqueues the launches on the current stream and returns (cam [B,h,w],
        heat [B,H,W], peak [B], heat_u8 [B,H,W] or None) as views of PINNED host buffers that the
        kernels write -- valid after the stream is synchronised and until the next call with the
        same (owner, plan shape, layer).  speed / command: the tensors the forward was given."""
        pl = self._followup_plan("run_gradcam")
        layer = int(layer)
        if not 1 <= layer <= 4:
            raise ValueError("layer must be in 1..4")
        w = self._gradcam_weights(weights4)

        def make():
            h, wd, ch = L.i32(), L.i32(), L.i32()
            L.check(L.lib().cilrs_net_gradcam_info(pl.handle, layer, None, None, C.byref(h),
                                                   C.byref(wd), C.byref(ch)))
            b, ncam, nheat = pl.batch, pl.batch * h.value * wd.value, pl.batch * pl.h * pl.w
            n = L.lib().cilrs_gradcam_scratch_floats(self.variant, b)
            scratch = torch.empty(n, dtype=torch.float32, device=self.device)
            host = torch.zeros(ncam + b + nheat, dtype=torch.float32).pin_memory()
            u8 = torch.zeros(nheat, dtype=torch.uint8).pin_memory().view(b, pl.h, pl.w)
            return (scratch, host, host[:ncam].view(b, h.value, wd.value), host[ncam:ncam + b],
                    host[ncam + b:].view(b, pl.h, pl.w), u8)
        scratch, _host, cam, peak, heat, u8 = self._followup_buffers(
            "gradcam", owner, (pl.batch, pl.h, pl.w, layer), make)
        L.check(L.lib().cilrs_net_gradcam(
            pl.handle, C.byref(pl.bufs), L.ptr(speed), L.ptr(command), w, layer, L.ptr(cam),
            L.ptr(heat), L.ptr(u8) if want_u8 else None, L.ptr(peak), L.ptr(scratch),
            scratch.numel(), self._stream()))
        return cam, heat, peak, (u8 if want_u8 else None)

    # ---- feature-space novelty (csrc/novelty.hip) --------------------------------------------------
    def feature_width(self) -> int:
        return int(L.lib().cilrs_variant_feature_width(self.variant))

    def plan_features(self, pl):
        """View [B, F] of the fp32 pooled features (`combined`) in a plan's workspace: what every
        eval-mode forward but the persistent single-frame launch leaves there."""
        co, ld, feat = L.sz(), L.i32(), L.i32()
        L.check(L.lib().cilrs_net_infer16_io_info(pl.handle, None, None, C.byref(co), C.byref(ld),
                                                  C.byref(feat)))
        comb = pl.workspace[co.value:co.value + 4 * pl.batch * ld.value].view(torch.float32)
        return comb.view(pl.batch, ld.value)[:, :feat.value]

    def run_feature_moments(self, command, pivot, table):
        """cilrs_net_feature_moments: add the pooled features the last eval-mode forward left in
        its plan, one row per frame, to the float64 moment table (include/cilrs_hip.h).  One
        launch on the current stream; nothing is copied to the host."""
        pl = self._followup_plan("run_feature_moments")
        L.check(L.lib().cilrs_net_feature_moments(
            pl.handle, C.byref(pl.bufs), L.ptr(command), L.ptr(pivot), L.ptr(table), self._stream()))

    def run_novelty(self, command, mean, W, d2=None, owner=None):
        """cilrs_net_novelty on the features the last eval-mode forward left in its plan: enqueues
        the three launches on the current stream and returns d2 [B].  Without `d2` the kernels
        write a PINNED host buffer, valid after the stream is synchronised and until the next call
        with the same (owner, B); the scratch is cached the same way (see run_heads_mc)."""
        pl = self._followup_plan("run_novelty")
        b = pl.batch

        def make():
            n = L.lib().cilrs_feature_novelty_scratch_floats(self.feature_width(), b)
            return (torch.empty(n, dtype=torch.float32, device=self.device),
                    torch.zeros(b, dtype=torch.float32).pin_memory())
        scratch, host = self._followup_buffers("novelty", owner, (b,), make)
        out = host if d2 is None else d2
        L.check(L.lib().cilrs_net_novelty(
            pl.handle, C.byref(pl.bufs), L.ptr(command), L.ptr(mean), L.ptr(W), L.ptr(out),
            L.ptr(scratch), scratch.numel(), self._stream()))
        return out

    def run_knn(self, rows, origin, W, k, owner=None):
        """cilrs_net_knn: the k rows of ``rows`` [N, F] (a NeighbourIndex's) nearest to the features
        the last eval-mode forward left in its plan, whitened by (origin, W) when given.  Enqueues
        the launches on the current stream and returns (idx int64 [B, k], dist float32 [B, k]) in
        PINNED host buffers, valid after the stream is synchronised and until the next call with
        the same (owner, B, k); the scratch is cached the same way (see run_novelty)."""
        pl = self._followup_plan("run_knn")
        b, n, k = pl.batch, rows.size(0), int(k)
        need = L.lib().cilrs_net_knn_scratch_bytes(self.feature_width(), b, n, k)

        def make():
            return (torch.empty(max(need, 16), dtype=torch.uint8, device=self.device),
                    torch.full((b, k), -1, dtype=torch.int64).pin_memory(),
                    torch.zeros(b, k, dtype=torch.float32).pin_memory())
        # (a pool that has grown since the entry was made needs longer lists: rebuilt)
        scratch, idx, dist = self._followup_buffers("knn", owner, (b, k), make,
                                                    lambda bufs: bufs[0].numel() >= need)
        L.check(L.lib().cilrs_net_knn(
            pl.handle, C.byref(pl.bufs), L.ptr(rows), rows.stride(0), n, L.ptr(origin), L.ptr(W), k,
            L.ptr(idx), L.ptr(dist), L.ptr(scratch), scratch.numel(), self._stream()))
        return idx, dist

    def run_forward_camera(self, frames_u8, speed, command, height=88, width=200, out=None):
        """Raw camera frames uint8 [B,Hs,Ws,3|4] (device) -> eval forward with the whole of
        preprocess_image fused: bilinear resize to (height, width), /255, normalise."""
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.size(3) not in (3, 4):
            raise RuntimeError("camera frames must be uint8 [B,Hs,Ws,3 or 4]")
        b = frames_u8.size(0)
        pl = self.plan(b, height, width)
        frames_u8 = frames_u8.contiguous()
        if out is None:
            controls = torch.empty(b, 3, dtype=torch.float32, device=self.device)
            pred_speed = torch.empty(b, dtype=torch.float32, device=self.device)
        else:
            controls, pred_speed = out
        hs, ws, px = frames_u8.size(1), frames_u8.size(2), frames_u8.size(3)
        self._announce_weights(pl)
        L.check(L.lib().cilrs_net_forward_camera(
            pl.handle, C.byref(pl.bufs), L.ptr(frames_u8), hs, ws, px,
            ws * px, hs * ws * px, L.ptr(speed.contiguous()), L.ptr(command.contiguous()),
            L.ptr(controls), L.ptr(pred_speed), self._stream()))
        self.last_plan = pl
        return controls, pred_speed

    def run_backward(self, pl, dcontrols, dpred_speed, seg_begin=0, seg_end=6, into=None,
                     data_only=False, segments=None):
        """Writes the parameter gradients of segments [seg_begin, seg_end) into the gradient
        arena, or into `into` (another arena of the same layout).  `segments` = (begin, end)
        overrides the two.  data_only=True: the data-gradient chain alone
        (cilrs_net_backward_data) -- no weight gradient is computed and no gradient arena is
        touched; run_input_grads follows it as usual."""
        if segments is not None:
            seg_begin, seg_end = segments
        if data_only:
            L.check(L.lib().cilrs_net_backward_data(
                pl.handle, C.byref(pl.bufs), L.ptr(dcontrols), L.ptr(dpred_speed), seg_begin,
                seg_end, self._stream()))
            return
        bufs = pl.bufs
        if into is not None:
            bufs = L.Buffers(self.params.data_ptr(), into.data_ptr(), self.bn.data_ptr(),
                             self.nbt.data_ptr(), pl.workspace.data_ptr())
        L.check(L.lib().cilrs_net_backward(
            pl.handle, C.byref(bufs), L.ptr(dcontrols), L.ptr(dpred_speed), seg_begin, seg_end,
            self._stream()))

    def run_input_grads(self, pl, dimage=None, dspeed=None):
        """After run_backward of the plan's last graph-keeping forward: d image (any strides)
        and / or d speed into the given tensors (None: not computed)."""
        if dimage is not None:
            if (dimage.dtype != torch.float32 or dimage.device != self.device or
                    tuple(dimage.shape) != (pl.batch, 3, pl.h, pl.w)):
                raise RuntimeError(f"dimage must be float32 [{pl.batch},3,{pl.h},{pl.w}] on "
                                   f"{self.device}")
            strides = dimage.stride()
        else:
            strides = (0, 0, 0, 0)
        if dspeed is not None and (dspeed.dtype != torch.float32 or tuple(dspeed.shape) != (pl.batch,)
                                   or not dspeed.is_contiguous() or dspeed.device != self.device):
            raise RuntimeError(f"dspeed must be a contiguous float32 [{pl.batch}] on {self.device}")
        L.check(L.lib().cilrs_net_input_grads(
            pl.handle, C.byref(pl.bufs), L.ptr(dimage) if dimage is not None else None, *strides,
            L.ptr(dspeed) if dspeed is not None else None, self._stream()))

    def run_backward_step(self, pl, dcontrols, dpred_speed, exp_avg, exp_avg_sq, lr, betas, eps,
                          weight_decay, step, grad_scale=1.0):
        """loss.backward() + Adam.step() in one library call (cilrs_net_backward_step): each
        segment's parameter range is updated as soon as its gradients are complete, under the
        remaining data gradients.  No gradient clipping on this path."""
        opt = L.AdamArgs(exp_avg.data_ptr(), exp_avg_sq.data_ptr(), float(lr), float(betas[0]),
                         float(betas[1]), float(eps), float(weight_decay), int(step),
                         float(grad_scale))
        self.weights_epoch += 1               # the update writes the parameter arena in place
        L.check(L.lib().cilrs_net_backward_step(
            pl.handle, C.byref(pl.bufs), L.ptr(dcontrols), L.ptr(dpred_speed), C.byref(opt),
            self._stream()))

    def grads_aliased(self) -> bool:
        """True when some parameter's .grad currently lives in the gradient arena (autograd kept
        a view handed out by an earlier backward)."""
        base = self.grads.untyped_storage().data_ptr()
        for p in self.module.parameters():
            g = p.grad
            if g is not None and g.untyped_storage().data_ptr() == base:
                return True
        return False

    # ------------------------------------------------------------------------------------------
    def forward(self, image, speed, command, training, dropout_p, seed):
        # a graph is built for train-mode steps with trainable parameters, and -- in either mode --
        # whenever an input asks for its gradient (eval mode: BatchNorm frozen on the running
        # statistics, as torch's own eval-mode autograd); otherwise the detached fast path
        grad_on = torch.is_grad_enabled()
        # train mode: the frozen prefix the module's flags describe (raises on what cannot be served)
        e = g = 0
        if training:
            e, g = self.module.freeze_state()
            self.check_freeze(e, g, image)
        needs_graph = grad_on and (image.requires_grad or speed.requires_grad)
        if not needs_graph:
            needs_graph = training and grad_on and any(
                p.requires_grad for p in self.module.parameters())
        if not needs_graph:
            if training:
                c, s, _ = self.run_forward_ft(image, speed, command, e, g, dropout_p, seed)
            else:
                c, s, _ = self.run_forward(image, speed, command, False, dropout_p, seed)
            return c, s
        params = tuple(self.module.parameters())
        gate = _ParamGate.apply(*params) if any(p.requires_grad for p in params) else None
        return _CILRSFunction.apply(self, image, speed, command, float(dropout_p), int(seed),
                                    bool(training), e, g, gate, *params)


_N_LEADING = 10       # _CILRSFunction.forward arguments in front of the parameters


class _ParamGate(torch.autograd.Function):
    """A node between the parameters and _CILRSFunction that computes nothing.  `needs_input_grad`
    of a custom Function is fixed when the graph is built (does the input require grad), whatever
    a later ``torch.autograd.grad(out, image)`` asks for; whether the autograd engine is going to
    run THIS node -- it leads to the parameters only -- says whether the pass under way wants any
    parameter gradient.  The gradients themselves go to the parameters directly, as before."""

    @staticmethod
    def forward(ctx, *params):
        ctx.set_materialize_grads(False)
        ctx.n = len(params)
        return params[0].new_empty(())

    @staticmethod
    def backward(ctx, _g):
        return (None,) * ctx.n


def _pass_wants_params(gate_node) -> bool:
    """Inside a backward: will the engine reach the parameters in this pass?  (True when it
    cannot be told: the full backward is always correct.)"""
    probe = getattr(torch._C, "_will_engine_execute_node", None)
    if gate_node is None or probe is None:
        return True
    try:
        return bool(probe(gate_node))
    except RuntimeError:
        return True


class _CILRSFunction(torch.autograd.Function):
    """Composable path: lets ``loss.backward()`` + any torch.optim drive the HIP engine
    (notebook/notebook.ipynb:549-555), and gives image.grad / speed.grad (saliency, sensitivity
    to the speed input) in train mode and -- through the frozen forward -- in eval mode."""

    @staticmethod
    def forward(ctx, eng, image, speed, command, dropout_p, seed, training, e, g, gate, *params):
        if training:
            controls, pred_speed, pl = eng.run_forward_ft(image, speed, command, e, g, dropout_p,
                                                          seed)
        else:
            controls, pred_speed, pl = eng.run_forward_frozen(image, speed, command)
        ctx.eng, ctx.pl, ctx.generation = eng, pl, pl.generation
        ctx.n_params = len(params)
        ctx.gate_node = gate.grad_fn if gate is not None else None
        ctx.frozen_groups = g if training else 0
        ctx.channels_last = (not image.is_contiguous()
                             and image.is_contiguous(memory_format=torch.channels_last))
        return controls, pred_speed

    @staticmethod
    def backward(ctx, dcontrols, dpred_speed):
        eng, pl = ctx.eng, ctx.pl
        if pl.generation != ctx.generation:
            raise RuntimeError(
                "CILRS backward: the saved activations of this forward were overwritten by a "
                "later train-mode forward (or eval-mode forward with an input requiring grad) "
                "with the same input shape (one graph per shape)")
        need_image, need_speed = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        # (parameters that require grad, AND a pass that asks for a parameter gradient:
        #  torch.autograd.grad(out, image) on a trainable model does not)
        need_params = any(ctx.needs_input_grad[_N_LEADING:]) and _pass_wants_params(ctx.gate_node)
        b = pl.batch
        if dcontrols is None:
            dcontrols = torch.zeros(b, 3, device=eng.device)
        if dpred_speed is None:
            dpred_speed = torch.zeros(b, device=eng.device)
        # torch semantics: what backward hands to autograd must stay valid for as long as anyone
        # holds it (autograd's own input buffers while several CILRS nodes of one graph are
        # summed, results of torch.autograd.grad, saved p.grad lists).  The kernels write into the
        # engine's gradient arena, which the NEXT backward overwrites -- so by default autograd
        # gets a clone (89.7 MB device copy, ~30 us).  `engine.zero_copy_grads = True` opts into
        # views of the arena for loops that consume the gradients before the next backward
        # (optimizer.step() + zero_grad(set_to_none=True)); when some p.grad still lives in the
        # arena that backward is written to a second arena instead, so accumulation stays correct.
        # (a backward for input gradients alone computes no parameter gradient at all: the
        #  data-gradient chain, down to the stem only when the image asks)
        dst = eng.grads
        if not need_params:
            eng.run_backward(pl, dcontrols.contiguous().float(), dpred_speed.contiguous().float(),
                             data_only=True, segments=(0, 6) if need_image else (0, 1))
        else:
            if eng.zero_copy_grads and eng.grads_aliased():
                if eng._scratch_grads is None:
                    eng._scratch_grads = torch.zeros_like(eng.grads)
                dst = eng._scratch_grads
            eng.run_backward(pl, dcontrols.contiguous().float(), dpred_speed.contiguous().float(),
                             into=None if dst is eng.grads else dst)
        dimage = dspeed = None
        if need_image or need_speed:
            if need_image:
                fmt = torch.channels_last if ctx.channels_last else torch.contiguous_format
                dimage = torch.empty((b, 3, pl.h, pl.w), dtype=torch.float32, device=eng.device,
                                     memory_format=fmt)
            if need_speed:
                dspeed = torch.empty(b, dtype=torch.float32, device=eng.device)
            eng.run_input_grads(pl, dimage, dspeed)
        lead = (None, dimage, dspeed) + (None,) * (_N_LEADING - 3)
        if not need_params:
            return lead + (None,) * ctx.n_params
        src = dst if eng.zero_copy_grads else dst.clone()
        # (the backward stopped at the frozen prefix: its arena range was not written)
        cut = eng.trainable_begin(ctx.frozen_groups)
        grads = [_arena_view(src, off, numel, shape) if off >= cut else None
                 for (_, off, numel, shape) in eng.params_layout]
        return (*lead, *grads)
