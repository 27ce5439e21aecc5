"""Fused training step -- the MI355X counterpart of the body of ``train_one_epoch``
(reference notebook/notebook.ipynb:545-558): forward, loss, backward, [clip], Adam, in that
order, all as HIP kernels on one stream with no host synchronisation (the reference's six
``.item()`` syncs per step, nb:523-526, become one device buffer read on demand).

Also the evaluation loop body (``validate``, nb:563-585) and StepLR (nb:535-536, 604).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from dataclasses import dataclass, field

import torch

from . import _lib as L

LOSS_KEYS = ("total", "control", "steer", "throttle", "brake", "speed")
CMD_NAMES = {0: "FOLLOW", 1: "LEFT", 2: "RIGHT", 3: "STRAIGHT"}


@dataclass
class TrainConfig:
    """A = documented config (README.md:98-108, configs/train_config.json:24-35; BASELINE.json);
    B = the config the notebook actually executed (notebook/notebook.ipynb:489-502)."""
    name: str = "A"
    lr: float = 2e-4
    weight_decay: float = 1e-4
    loss: str = "mse"                                  # "mse" | "l1"
    loss_weights: tuple = (1.0, 1.0, 1.0, 0.05)        # steer, throttle, brake, speed
    grad_clip: float = 0.0
    dropout: float = 0.0
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    lr_step_size: int = 8
    lr_gamma: float = 0.5
    # fine-tuning: learning-rate multiplier per parameter group ("stem", "layer1" .. "layer4",
    # "heads"; missing = 1.0) -- the lower trunk rate that is usual on top of a pretrained trunk.
    # None, or all 1.0: the step is the single-rate step, launch for launch.
    lr_mult: dict = None
    # exponential moving average of the weights, updated on every optimizer step by a streaming
    # pass behind the Adam launch (Trainer.ema; Trainer.ema_fused moves it into the launch;
    # include/cilrs_hip.h "exponential moving average"): the decay d, 0 <= d < 1;
    # None = off, and then no launch, file or checkpoint differs.  ema_warmup: the decay of update
    # t (1-based) is min(d, (1 + t) / (10 + t)), so that the first steps are not averaged with the
    # initialisation at full weight.
    ema_decay: float = None
    ema_warmup: bool = True
    # the update rule (include/cilrs_hip.h "AdamW and LAMB"): "adam" = torch.optim.Adam with coupled
    # L2 decay, the reference's; "adamw" = decoupled decay; "lamb" = layer-wise adaptive, one trust
    # ratio per parameter tensor.  The moments have one layout in all three.
    optimizer: str = "adam"
    # every tensor with ndim <= 1 (BatchNorm weight and bias, Linear bias) takes no weight decay
    # and, under "lamb", the trust ratio 1.  Not with "adam" (its decay is one scalar per launch).
    decay_exempt_1d: bool = False
    trust_clip: float = 0.0                            # LAMB: ||p|| is capped here; 0 = off
    # the rate of optimizer step t (1-based) is lr * min(1, t / warmup_steps); 0 = off
    warmup_steps: int = 0
    lr_schedule: str = "step"                          # "step" (StepLR) | "cosine"
    lr_epochs: int = 20                                # cosine: epochs down to lr_min
    lr_min: float = 0.0
    # sharpness-aware minimisation (include/cilrs_hip.h "sharpness-aware minimisation"): the step's
    # gradient is taken at w + e(w), |e| = sam_rho along the gradient at w (sam_adaptive: ASAM, the
    # scale-invariant form), and applied at w -- two forward / backward passes per step.  0 = off,
    # and then no launch, buffer or checkpoint differs.  sam_every: SAM runs on the optimizer steps
    # t (1-based) with (t - 1) % sam_every == 0, the plain step on the others.
    sam_rho: float = 0.0
    sam_adaptive: bool = False
    sam_every: int = 1
    # adversarial training (include/cilrs_hip.h "adversarial robustness"): the step is taken on
    # x_adv = the batch moved by one signed-gradient step of adv_alpha 8-bit levels (FGSM), from a
    # uniform random start in the eps ball when adv_random_start, kept within adv_eps levels of the
    # clean batch -- one extra forward / data-gradient pass per due step.  adv_eps = 0: off, and then
    # the step is launch for launch what it was.  adv_alpha None: 1.25 * adv_eps with a random
    # start, else adv_eps.  adv_every: the optimizer steps t (1-based) with (t - 1) % adv_every == 0
    # are adversarial.  adv_clamp: x_adv also stays inside the images of the bytes 0..255.
    adv_eps: float = 0.0
    adv_alpha: float = None
    adv_random_start: bool = True
    adv_every: int = 1
    adv_clamp: bool = False


GROUP_NAMES = ("stem", "layer1", "layer2", "layer3", "layer4", "heads")


def dropout_seed(torch_seed: int, call: int, rank: int = 0) -> int:
    """64-bit key of one forward's dropout masks (cilrs_net_forward `seed`)."""
    return ((torch_seed * 1000003 + call) ^ (rank * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF


def steplr(cfg: TrainConfig, epoch: int) -> float:
    """lr in effect AFTER `epoch` scheduler steps of torch.optim.lr_scheduler.StepLR(step_size,
    gamma) (nb:535-536: StepLR(8, 0.5), stepped once per epoch, nb:604)."""
    return cfg.lr * (cfg.lr_gamma ** (epoch // cfg.lr_step_size))


def cosine_lr(cfg: TrainConfig, epoch: int) -> float:
    """lr in effect AFTER `epoch` scheduler steps of the cosine schedule: from cfg.lr at epoch 0 down
    to cfg.lr_min at cfg.lr_epochs, where it stays."""
    e = min(int(epoch), int(cfg.lr_epochs))
    return cfg.lr_min + 0.5 * (cfg.lr - cfg.lr_min) * (1.0 + math.cos(math.pi * e / cfg.lr_epochs))


def scheduled_lr(cfg: TrainConfig, epoch: int) -> float:
    return cosine_lr(cfg, epoch) if cfg.lr_schedule == "cosine" else steplr(cfg, epoch)


def warmup_factor(warmup_steps: int, t: int) -> float:
    """min(1, t / warmup_steps) for optimizer step t (1-based); 1 with the warm-up off."""
    if warmup_steps <= 0 or t >= warmup_steps:
        return 1.0
    return max(t, 1) / float(warmup_steps)


OPTIMIZERS = ("adam", "adamw", "lamb")
SEG_NO_DECAY, SEG_NO_ADAPT = 1, 2                      # CILRS_SEG_* of include/cilrs_hip.h
OPTIM_KIND = {"adamw": 1, "lamb": 2}                   # CILRS_OPTIM_*


def check_optim_config(cfg: TrainConfig):
    """ValueError for what no Trainer can serve, before anything is built."""
    if cfg.optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {cfg.optimizer!r}")
    if cfg.lr_schedule not in ("step", "cosine"):
        raise ValueError(f"lr_schedule must be 'step' or 'cosine', got {cfg.lr_schedule!r}")
    if not (isinstance(cfg.warmup_steps, int) and cfg.warmup_steps >= 0):
        raise ValueError(f"warmup_steps must be an integer >= 0, got {cfg.warmup_steps!r}")
    if not (isinstance(cfg.trust_clip, (int, float)) and math.isfinite(cfg.trust_clip)
            and cfg.trust_clip >= 0):
        raise ValueError(f"trust_clip must be finite and >= 0 (0 = off), got {cfg.trust_clip!r}")
    if cfg.decay_exempt_1d and cfg.optimizer == "adam":
        raise ValueError("decay_exempt_1d has no effect with optimizer='adam' (its coupled decay is "
                         "one scalar for the whole launch); use 'adamw' or 'lamb'")
    if cfg.lr_schedule == "cosine":
        if not (isinstance(cfg.lr_epochs, int) and cfg.lr_epochs >= 1):
            raise ValueError(f"lr_epochs must be an integer >= 1, got {cfg.lr_epochs!r}")
        if not (math.isfinite(cfg.lr_min) and 0.0 <= cfg.lr_min <= cfg.lr):
            raise ValueError(f"lr_min must lie in [0, lr], got {cfg.lr_min!r}")
    check_sam_rho(cfg.sam_rho)
    if not (isinstance(cfg.sam_every, int) and not isinstance(cfg.sam_every, bool)
            and cfg.sam_every >= 1):
        raise ValueError(f"sam_every must be an integer >= 1, got {cfg.sam_every!r}")
    check_adv_config(cfg)


def check_adv_config(cfg: TrainConfig):
    """ValueError for an adversarial-training configuration no Trainer can serve."""
    for name in ("adv_eps", "adv_alpha"):
        v = getattr(cfg, name)
        if name == "adv_alpha" and v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be finite and >= 0 (8-bit levels), got {v!r}")
    for name in ("adv_random_start", "adv_clamp"):
        if not isinstance(getattr(cfg, name), bool):
            raise ValueError(f"{name} must be True or False, got {getattr(cfg, name)!r}")
    if not (isinstance(cfg.adv_every, int) and not isinstance(cfg.adv_every, bool)
            and cfg.adv_every >= 1):
        raise ValueError(f"adv_every must be an integer >= 1, got {cfg.adv_every!r}")
    if cfg.adv_eps > 0 and cfg.sam_rho > 0:
        raise ValueError("adv_eps > 0 together with sam_rho > 0: both take the step's extra pass "
                         "(perturb the input or the weights, not both)")


def adv_alpha(cfg: TrainConfig) -> float:
    """The adversarial step in 8-bit levels: adv_alpha, or 1.25 * adv_eps with a random start and
    adv_eps without."""
    if cfg.adv_alpha is not None:
        return float(cfg.adv_alpha)
    return 1.25 * float(cfg.adv_eps) if cfg.adv_random_start else float(cfg.adv_eps)


def adv_step_due(adv_every: int, t: int) -> bool:
    """Is optimizer step t (1-based) adversarial?  Steps 1, 1 + adv_every, 1 + 2 adv_every, ..."""
    return (int(t) - 1) % int(adv_every) == 0


def adv_seed(torch_seed: int, call: int, rank: int = 0) -> int:
    """64-bit key of the random start of the `call`-th adversarial step (cilrs_adv_start `seed`)."""
    return ((torch_seed * 1000033 + call) ^ (rank * 0x9E3779B97F4A7C15) ^ 0xAD5EED) \
        & 0xFFFFFFFFFFFFFFFF


def check_sam_rho(rho):
    """float(rho) if it is a usable SAM radius (finite, >= 0; 0 = off), else ValueError."""
    if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not math.isfinite(rho) \
            or rho < 0:
        raise ValueError(f"sam_rho must be finite and >= 0 (0 = off), got {rho!r}")
    return float(rho)


def segment_table(params_layout, n_arena, decay_exempt_1d=False, lamb=False):
    """(ends, flags) of the optimizer's segment table: one segment per parameter tensor, from its
    arena offset to the next tensor's (the last one to the arena's end).  decay_exempt_1d: tensors
    with ndim <= 1 carry NO_DECAY, and NO_ADAPT too under LAMB."""
    offs = [p[1] for p in params_layout]
    if not offs or offs[0] != 0 or any(b <= a for a, b in zip(offs, offs[1:])):
        raise RuntimeError("parameter layout does not start at 0 with increasing offsets")
    ends = offs[1:] + [int(n_arena)]
    exempt = SEG_NO_DECAY | (SEG_NO_ADAPT if lamb else 0)
    flags = [exempt if decay_exempt_1d and len(p[3]) <= 1 else 0 for p in params_layout]
    return ends, flags


def sam_step_due(sam_every: int, t: int) -> bool:
    """Is optimizer step t (1-based) a SAM step?  Steps 1, 1 + sam_every, 1 + 2 sam_every, ..."""
    return (int(t) - 1) % int(sam_every) == 0


def ema_decay_at(decay: float, t: int, warmup: bool = True) -> float:
    """Decay of the t-th EMA update (1-based), in double."""
    d = float(decay)
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def ema_weight(decay: float, t: int, warmup: bool = True) -> float:
    """w of `ema = ema + w * (p - ema)` for update t: 1 - d_t in double, rounded to fp32 once."""
    return C.c_float(1.0 - ema_decay_at(decay, t, warmup)).value


def check_ema_decay(decay):
    """float(decay) if it is a usable decay (finite, 0 <= d < 1), else ValueError."""
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"ema_decay must be a number in [0, 1) or None, got {decay!r}") from None
    if not (math.isfinite(d) and 0.0 <= d < 1.0):
        raise ValueError(f"ema_decay must be finite and in [0, 1), got {decay!r}")
    return d


CONFIG_A = TrainConfig()
CONFIG_B = TrainConfig(name="B", lr=1e-4, loss="l1", loss_weights=(5.0, 1.0, 1.0, 0.5),
                       grad_clip=1.0, dropout=0.5)


class Trainer:
    def __init__(self, model, cfg: TrainConfig = CONFIG_A, process_group=None, precision="fp32"):
        """precision="bf16": BASELINE.json configs[3]'s "bf16 MFMA path" -- the trunk convolutions
        of the train step multiply bf16 operands (fp32 accumulation); master weights, BatchNorm,
        heads, loss and Adam stay fp32.  Not the reference's arithmetic: agrees with the fp32 step
        to bf16 rounding, not to 1e-4."""
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        ema_decay = None if cfg.ema_decay is None else check_ema_decay(cfg.ema_decay)
        check_optim_config(cfg)
        self.model = model
        self.cfg = cfg
        self.eng = model.engine()
        self.eng.train_precision = precision
        dev = self.eng.device
        n = self.eng.n_arena
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_count = 0
        # Adam's bias correction counts a tensor's OWN updates (torch.optim.Adam keeps `step` per
        # parameter and skips `grad is None`): steps each parameter group sat out while frozen.
        # A group's step is step_count - group_lag[i]; with nothing ever frozen all six are equal.
        self.group_lag = [0] * 6
        mult = dict(cfg.lr_mult or {})
        unknown = set(mult) - set(GROUP_NAMES)
        if unknown:
            raise ValueError(f"lr_mult: unknown group(s) {sorted(unknown)}; one of {GROUP_NAMES}")
        self.lr_mult = [float(mult.get(n, 1.0)) for n in GROUP_NAMES]
        self.epoch = 0
        self.lr = cfg.lr
        self.loss_buf = torch.zeros(8, dtype=torch.float32, device=dev)
        self.clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
        self.norm_scratch = torch.empty(L.lib().cilrs_sqnorm_scratch_bytes(), dtype=torch.uint8,
                                        device=dev)
        self._dgrads = {}
        self._w = (C.c_float * 4)(*cfg.loss_weights)
        self._kind = 1 if cfg.loss == "l1" else 0
        self._seed_calls = 0
        self.rows_calls = 0                    # launches of cilrs_loss_fwd_bwd_rows (Trainer.loss)
        self.arena_grad_scale = 1.0
        # True: single-GPU steps without clipping take cilrs_net_backward_step (a segment's Adam
        # update enqueued behind its gradients, on the weight-gradient stream) instead of backward +
        # one Adam launch over the arena -- the same numbers, element by element.  Off by default:
        # the overlapped step is bound by the kernels' resource time, not by its critical path,
        # and the six extra stream forks cost more than the overlap gains (9.24 vs 9.215 ms,
        # tools/dp_overhead.sh).
        self.fuse_optimizer = False
        # data parallel without clipping: Adam per all-reduce bucket as soon as the bucket's
        # averaged gradient is there (the last, small bucket's collective runs under the first two
        # buckets' updates)
        self.bucket_optimizer = True
        # EMA of the weights: fp32 over the fp32 master arena in every precision mode, a copy of the
        # parameters now.  BatchNorm buffers are not averaged (running statistics already are
        # moving averages): until update_bn(ema=True) has run, the averaged weights are evaluated
        # with the live model's buffers; from then on with buffers of their own (ema_bn / ema_nbt,
        # re-estimated on the averaged weights and exchanged together with the parameters).
        self.ema_decay = ema_decay
        self.ema = self.eng.params.clone() if ema_decay is not None else None
        self.ema_bn = None
        self.ema_nbt = None
        self.ema_updates = 0
        # False: Adam, then cilrs_ema_update over the same range; True: the average is updated
        # inside the Adam launch (cilrs_adam_step_ema) -- the same numbers bit for bit.  By bytes
        # the fused launch should win (9 arena-sized arrays against 10 and a launch); measured it
        # does not: 0.157 ms against 0.147 ms over the arena (Adam alone 0.107; a hypothesis, no
        # counters taken: the separate pass finds the parameters Adam has just written in the
        # last-level cache).  In the B=128 step the fused route reads 0.022 ms faster, inside the
        # larger spread of 0.025 ms (profiles/ema_bench.log).  By the rule
        # set before measuring -- fused only if it wins over the arena -- the separate pass is
        # the default.
        self.ema_fused = False
        self._ema_w = 0.0
        self._in_ema = False
        # AdamW / LAMB: the segment table (one segment per parameter tensor) on the device, built
        # once; LAMB's partial sums and the per-tensor trust ratios of the last step
        self._optim_table = None
        if cfg.optimizer != "adam":
            self._build_optim_table()
        # SAM: the arena-sized copy of the weights a step starts from, the chunk sums and
        # {S, norm, scale} of the last perturbation, the loss at w + e.  With sam_rho == 0 only
        # the 32-byte loss buffer exists (Trainer.sharpness creates the others on first use).
        self.sam_backup = None
        self._sam_scratch = None
        self._sam_out3 = None
        self.sam_loss_buf = torch.zeros(8, dtype=torch.float32, device=dev)
        self.sam_steps = 0
        self._bn_snapshot = None
        if cfg.sam_rho > 0:
            self._sam_buffers()
        # adversarial training: batch-sized x_adv / image-gradient buffers (made on first use, in the
        # images' strides) and the count of adversarial steps taken
        self._adv_bufs = {}
        self.adv_steps = 0
        self.reducer = None
        self.rank = 0
        if process_group is not None:
            import torch.distributed as dist
            from .parallel import BucketedAllReduce
            self.reducer = BucketedAllReduce(self.eng.grads, process_group,
                                             variant=self.eng.variant)
            self.rank = dist.get_rank(process_group)

    # -- AdamW / LAMB ---------------------------------------------------------------------------
    def _build_optim_table(self):
        lib, eng, cfg = L.lib(), self.eng, self.cfg
        ends, flags = segment_table(eng.params_layout, eng.n_arena, cfg.decay_exempt_1d,
                                    cfg.optimizer == "lamb")
        k = len(ends)
        c_ends, c_flags = (C.c_size_t * k)(*ends), (C.c_int * k)(*flags)
        nbytes = lib.cilrs_optim_table_bytes(c_ends, k)
        if nbytes == 0:
            raise RuntimeError("cilrs_optim_table_bytes refused the parameter layout")
        self._seg_ends = ends
        self._seg_index_of_start = {b: i for i, b in enumerate([0] + ends[:-1])}
        self._seg_index_of_end = {e: i for i, e in enumerate(ends)}
        self._optim_table_mem = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
        handle = C.c_void_p()
        L.check(lib.cilrs_optim_table_create(c_ends, c_flags, k, eng.n_arena,
                                             L.ptr(self._optim_table_mem), nbytes, self._stream(),
                                             C.byref(handle)))
        self._optim_table = handle
        self._optim_scratch = torch.empty(max(lib.cilrs_optim_scratch_bytes(handle), 16),
                                          dtype=torch.uint8, device=eng.device)
        self._ratios = torch.ones(k, dtype=torch.float32, device=eng.device)

    def __del__(self):
        handle = getattr(self, "_optim_table", None)
        if handle is not None:
            self._optim_table = None
            try:
                L.lib().cilrs_optim_table_destroy(handle)
            except Exception:
                pass

    def trust_ratios(self):
        """LAMB's trust ratio r_s of every parameter tensor at its last update (1 before the first
        one, and always for NO_ADAPT tensors): a CPU fp32 tensor in params_layout order."""
        if self.cfg.optimizer != "lamb":
            raise RuntimeError("trust ratios exist under optimizer='lamb' only")
        return self._ratios.detach().cpu().clone()

    def lr_at(self, t):
        """Learning rate of optimizer step t (1-based): the scheduled per-epoch `lr` times the
        warm-up factor min(1, t / warmup_steps)."""
        f = warmup_factor(self.cfg.warmup_steps, t)
        return self.lr if f == 1.0 else self.lr * f

    @property
    def lr_now(self):
        """The effective rate of optimizer step `step_count` (before the first step: of step 1)."""
        return self.lr_at(max(self.step_count, 1))

    def _refuse_unserved_optimizer(self):
        if self.cfg.sam_rho > 0 and self.fuse_optimizer:
            raise RuntimeError("Trainer.fuse_optimizer cannot serve sam_rho: cilrs_net_backward_"
                               "step updates a segment's weights under the remaining data "
                               "gradients, before the perturbation can be taken back (leave "
                               "fuse_optimizer off, the default)")
        if self.cfg.optimizer == "adam":
            return
        if self.fuse_optimizer:
            raise RuntimeError(f"Trainer.fuse_optimizer cannot serve optimizer={self.cfg.optimizer!r}"
                               ": cilrs_net_backward_step's per-segment launches are Adam's (leave "
                               "fuse_optimizer off, the default)")
        if self.ema_fused:
            raise RuntimeError(f"Trainer.ema_fused cannot serve optimizer={self.cfg.optimizer!r}: "
                               "only the Adam launches carry the average (leave ema_fused off, the "
                               "default; the separate cilrs_ema_update pass follows the step)")

    # -- pieces ---------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.eng.device).cuda_stream)

    def _ensure_engine(self):
        eng = self.model.engine()
        if eng is not self.eng:
            raise RuntimeError("the model was moved/re-created after the Trainer was built")
        return eng

    def loss(self, controls, targets, pred_speed, target_speed, want_grads=True, out=None,
             sample_weight=None, row_loss=None):
        """CILRSLoss (nb:514-527) / the documented MSE loss; returns device buffer [6] in
        LOSS_KEYS order, plus (dcontrols, dpred_speed) when want_grads.  out: the fp32 device
        buffer (>= 6) the terms are written to instead of `loss_buf`.

        sample_weight (device fp32 [B]): every sample's gradient is multiplied by its weight and
        the terms are the weighted means; row_loss (device fp32 [B]): receives the unweighted
        per-sample losses.  With either one the launch is cilrs_loss_fwd_bwd_rows (`rows_calls`
        counts them), with neither it is cilrs_loss_fwd_bwd as ever."""
        out = self.loss_buf if out is None else out
        b = controls.size(0)
        dc = dp = None
        if want_grads:
            if b not in self._dgrads:
                self._dgrads[b] = (torch.empty(b, 3, device=controls.device),
                                   torch.empty(b, device=controls.device))
            dc, dp = self._dgrads[b]
        if sample_weight is not None or row_loss is not None:
            for name, t in (("sample_weight", sample_weight), ("row_loss", row_loss)):
                if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (b,)
                                      or t.device != controls.device or not t.is_contiguous()):
                    raise ValueError(f"{name} must be a contiguous fp32 [{b}] tensor on the "
                                     "model's device")
            self.rows_calls += 1
            L.check(L.lib().cilrs_loss_fwd_bwd_rows(
                L.ptr(controls), L.ptr(targets.contiguous()), L.ptr(pred_speed),
                L.ptr(target_speed.contiguous()), b, self._kind, self._w, 1.0, L.ptr(dc), L.ptr(dp),
                L.ptr(out), L.ptr(sample_weight), L.ptr(row_loss), self._stream()))
            return out, dc, dp
        L.check(L.lib().cilrs_loss_fwd_bwd(
            L.ptr(controls), L.ptr(targets.contiguous()), L.ptr(pred_speed),
            L.ptr(target_speed.contiguous()), b, self._kind, self._w, 1.0, L.ptr(dc), L.ptr(dp),
            L.ptr(out), self._stream()))
        return out, dc, dp

    @property
    def group_steps(self):
        """Adam step count of each parameter group (GROUP_NAMES order)."""
        return [self.step_count - lag for lag in self.group_lag]

    def _freeze_state(self):
        """The module's (e, g) (CILRS.freeze_state), refused where this Trainer cannot serve it."""
        e, g = self.model.freeze_state()
        self.eng.check_freeze(e, g)
        return e, g

    def _advance_steps(self, frozen_groups):
        """One optimizer step begins: the trainable groups count it, the frozen ones sit it out.
        With EMA on it is also one EMA update: its weight is fixed here, once, for every range the
        step updates, and the frozen prefix -- which no Adam launch visits -- is averaged by a
        pass of its own (a group that was trained, then frozen, keeps converging to its
        parameters; where ema == p already the pass changes nothing)."""
        self.step_count += 1
        for i in range(frozen_groups):
            self.group_lag[i] += 1
        if self.ema is None:
            return
        self.ema_updates += 1
        self._ema_w = ema_weight(self.ema_decay, self.ema_updates, self.cfg.ema_warmup)
        begin = self.eng.trainable_begin(frozen_groups)
        if begin > 0:
            self._ema_pass(0, begin)

    def _ema_pass(self, b, e):
        L.check(L.lib().cilrs_ema_update(L.ptr(self.ema[b:e]), L.ptr(self.eng.params[b:e]), e - b,
                                         self._ema_w, self._stream()))

    def _refuse_inside_ema_weights(self, what):
        if self._in_ema:
            raise RuntimeError(f"Trainer.{what} inside `with trainer.ema_weights():` -- the arena "
                               "holds the averaged weights there; leave the context first")

    def optimizer_step(self, grad_scale=1.0):
        """clip_grad_norm_ (nb:553-554) + Adam.step (nb:555) over the flat arena -- over its
        trainable range when a prefix of the trunk is frozen (frozen parameters and their moments
        are not touched and take no weight decay, like torch.optim.Adam's `grad is None`)."""
        self._refuse_inside_ema_weights("optimizer_step")
        self._refuse_unserved_optimizer()
        lib = L.lib()
        eng, cfg = self.eng, self.cfg
        e, g = self._freeze_state()
        begin = eng.trainable_begin(g)
        n = eng.n_arena - begin
        clip_ptr = None
        # arena * arena_grad_scale = the (rank-averaged) gradient this step's clip + Adam consume
        self.arena_grad_scale = 1.0 if cfg.grad_clip > 0 else float(grad_scale)
        if cfg.grad_clip > 0:
            if grad_scale != 1.0:
                L.check(lib.cilrs_scale(L.ptr(eng.grads[begin:]), n, None, grad_scale,
                                        self._stream()))
                grad_scale = 1.0
            L.check(lib.cilrs_grad_sqnorm(L.ptr(eng.grads[begin:]), n, cfg.grad_clip,
                                          L.ptr(self.norm_scratch), L.ptr(self.clip_out),
                                          self._stream()))
            clip_ptr = L.ptr(self.clip_out)
        self._advance_steps(g)
        eng.wrote_trainable(e)                # the fused Adam writes the parameter arena in place
        self._adam_range(begin, eng.n_arena, grad_scale, clip_ptr, g)

    # -- one iteration of train_one_epoch's loop (nb:549-555) ------------------------------------
    def train_step(self, imgs, speeds, cmds, tgts, sample_weight=None, row_loss=None):
        """Returns the device loss buffer [>=6] (LOSS_KEYS order); reading it is the only sync.

        sample_weight / row_loss (device fp32 [B], `Trainer.loss`): importance weights on the
        samples' gradients, and where the step's unweighted per-sample losses go -- what a
        `PrioritizedBatchLoader` gives and takes.  Under SAM the weights apply to both passes and
        row_loss is the first pass's (the loss at w).  With both None the step is launch for
        launch what it always was."""
        self._refuse_inside_ema_weights("train_step")
        self._refuse_unserved_optimizer()
        if self.ema is not None and self.fuse_optimizer:
            raise RuntimeError("Trainer.fuse_optimizer cannot serve ema_decay: cilrs_net_backward_"
                               "step's per-segment Adam launches carry no average (leave "
                               "fuse_optimizer off, the default)")
        eng = self._ensure_engine()
        if not self.model.training:
            self.model.train()
        # the frozen prefix the module's flags describe, re-read on every step (raises on a
        # pattern that cannot be served, before any launch)
        e, g = self._freeze_state()
        if g and self.reducer is None and self.cfg.grad_clip <= 0 and self.fuse_optimizer:
            raise RuntimeError("Trainer.fuse_optimizer cannot serve a frozen trunk prefix (one "
                               "fused update per backward segment, one step count)")
        adv = self.cfg.adv_eps > 0 and adv_step_due(self.cfg.adv_every, self.step_count + 1)
        if adv:
            self._refuse_unserved_adversarial(e, g)
        seed = self.next_dropout_seed() if self.cfg.dropout > 0 else 0
        if adv:
            # (row_loss is the first pass's, like SAM's: the loss of the batch as it was drawn)
            imgs = self._adversarial_batch(imgs, speeds, cmds, tgts, seed, sample_weight, row_loss)
            row_loss = None
        controls, pred_speed, pl = eng.run_forward_ft(imgs, speeds, cmds, e, g, self.cfg.dropout,
                                                      seed)
        # `speeds` is both an input and the speed head's regression target (nb:550)
        _, dc, dp = self.loss(controls, tgts, pred_speed, speeds, sample_weight=sample_weight,
                              row_loss=row_loss)
        sam = self.cfg.sam_rho > 0 and sam_step_due(self.cfg.sam_every, self.step_count + 1)
        if sam:
            pl, dc, dp = self._sam_second_pass(pl, dc, dp, imgs, speeds, cmds, tgts, e, g, seed,
                                               sample_weight)
        if self.reducer is None and self.cfg.grad_clip <= 0 and self.fuse_optimizer:
            # backward + Adam in one call: a segment's update runs as soon as its gradients are
            # complete (clipping needs the global norm first and keeps the two-call path below)
            if len(set(self.lr_mult)) != 1 or len(set(self.group_lag)) != 1:
                raise RuntimeError("Trainer.fuse_optimizer takes one learning rate and one step "
                                   "count for the whole arena (lr_mult / earlier frozen steps)")
            self._advance_steps(0)
            self.arena_grad_scale = 1.0
            eng.run_backward_step(pl, dc, dp, self.exp_avg, self.exp_avg_sq,
                                  self.lr_now * self.lr_mult[0], self.cfg.betas, self.cfg.eps,
                                  self.cfg.weight_decay, self.group_steps[0])
        elif self.reducer is None:
            eng.run_backward(pl, dc, dp)
            if sam:
                self._sam_restore(e, g)
            self.optimizer_step(1.0)
        elif self.cfg.grad_clip <= 0 and self.bucket_optimizer:
            # data parallel without clipping: Adam per all-reduce bucket, as soon as the bucket's
            # averaged gradient is there (the last bucket's collective runs under the first two
            # buckets' updates); same numbers as one launch over the arena
            self._advance_steps(g)
            eng.wrote_trainable(e)
            scale = 1.0 / self.reducer.world_size
            self.arena_grad_scale = scale
            pending = [sam]       # SAM: w comes back before the first bucket's update (every
                                  # backward segment is enqueued by then: they read w + e)

            def after_bucket(_i, b, e_):
                if pending[0]:
                    pending[0] = False
                    self._sam_restore(e, g)
                self._adam_range(b, e_, scale, None, g)
            self.reducer.backward_and_reduce(eng, pl, dc, dp, frozen_groups=g,
                                             after_bucket=after_bucket)
        else:
            self.reducer.backward_and_reduce(eng, pl, dc, dp, frozen_groups=g)
            if sam:
                self._sam_restore(e, g)
            self.optimizer_step(1.0 / self.reducer.world_size)
        return self.loss_buf

    # -- adversarial training ----------------------------------------------------------------------
    def _refuse_unserved_adversarial(self, e, g):
        if g:
            from .engine import SEG_NAMES
            raise RuntimeError("CILRS adversarial training: the trunk is frozen up to "
                               f"{SEG_NAMES[6 - g]} and the image gradient stops at the cut "
                               "(unfreeze the trunk, or set adv_eps = 0)")
        if self.eng.train_precision != "fp32":
            raise RuntimeError("CILRS adversarial training: fp32 plans only (the image gradient of "
                               f"the {self.eng.train_precision} training plan is not served)")

    def _adversarial_batch(self, imgs, speeds, cmds, tgts, seed, sample_weight, row_loss):
        """x_adv of a due step: random start, a train-mode forward with the
        step's dropout masks, the loss, the data-gradient-only backward, the image gradient, one
        signed step.  No collective: like SAM's first pass the perturbation is per rank.  The
        running BatchNorm statistics and num_batches_tracked are put back, so the step ends as ONE
        forward on x_adv leaves them."""
        from .adversarial import CHAN_SCALE, RANGE6
        eng, cfg = self.eng, self.cfg
        key = (tuple(imgs.shape), tuple(imgs.stride()))
        if key not in self._adv_bufs:
            self._adv_bufs = {key: (torch.empty_strided(imgs.shape, imgs.stride(),
                                                        dtype=torch.float32, device=imgs.device),
                                    torch.empty_strided(imgs.shape, imgs.stride(),
                                                        dtype=torch.float32, device=imgs.device))}
        x_adv, grad = self._adv_bufs[key]
        range6 = RANGE6 if cfg.adv_clamp else None
        if self._bn_snapshot is None:
            self._bn_snapshot = (torch.empty_like(eng.bn), torch.empty_like(eng.nbt))
        self.adv_steps += 1
        eng.snapshot_bn(*self._bn_snapshot)
        eng.run_adv_start(imgs, cfg.adv_eps if cfg.adv_random_start else 0.0, CHAN_SCALE,
                          adv_seed(torch.initial_seed(), self.adv_steps, self.rank), x_adv, range6)
        controls, pred_speed, pl = eng.run_forward_ft(x_adv, speeds, cmds, 0, 0, cfg.dropout, seed)
        _, dc, dp = self.loss(controls, tgts, pred_speed, speeds, out=self.sam_loss_buf,
                              sample_weight=sample_weight, row_loss=row_loss)
        eng.run_backward(pl, dc, dp, data_only=True)
        eng.run_input_grads(pl, grad, None)      # (a plan that cannot give it refuses here)
        eng.run_adv_step(imgs, x_adv, grad, adv_alpha(cfg), cfg.adv_eps, CHAN_SCALE, None, None,
                         None, range6)
        eng.put_back_bn(*self._bn_snapshot)
        return x_adv

    # -- sharpness-aware minimisation --------------------------------------------------------------
    def _sam_buffers(self):
        """The backup arena, the chunk-sum scratch and out3 (its last three doubles), once."""
        if self.sam_backup is None:
            eng = self.eng
            nbytes = L.lib().cilrs_sam_scratch_bytes(eng.n_arena)
            if nbytes == 0:
                raise RuntimeError("cilrs_sam_scratch_bytes refused the arena size")
            self.sam_backup = torch.empty(eng.n_arena, dtype=torch.float32, device=eng.device)
            self._sam_scratch = torch.zeros(nbytes // 8, dtype=torch.float64, device=eng.device)
            self._sam_out3 = self._sam_scratch[nbytes // 8 - 3:]
        return self.sam_backup

    def _sam_perturb(self, e, g, rho, adaptive):
        """w -> w + e(w) over the trainable range from the gradient arena as it stands; the write
        is announced like Adam's (Winograd transforms, bf16 copies and a frozen prefix's cached
        state behave as after an optimizer step)."""
        eng = self.eng
        backup = self._sam_buffers()
        begin = eng.trainable_begin(g)
        L.check(L.lib().cilrs_sam_perturb(
            L.ptr(eng.params[begin:]), L.ptr(eng.grads[begin:]), L.ptr(backup[begin:]),
            eng.n_arena - begin, float(rho), 1 if adaptive else 0, L.ptr(self._sam_scratch),
            L.ptr(self._sam_out3), self._stream()))
        eng.wrote_trainable(e)

    def _sam_restore(self, e, g):
        """w + e -> w, bit for bit (cilrs_sam_restore), announced like the perturbation."""
        eng = self.eng
        begin = eng.trainable_begin(g)
        L.check(L.lib().cilrs_sam_restore(L.ptr(eng.params[begin:]), L.ptr(self.sam_backup[begin:]),
                                          eng.n_arena - begin, self._stream()))
        eng.wrote_trainable(e)

    def _sam_second_pass(self, pl, dc, dp, imgs, speeds, cmds, tgts, e, g, seed,
                         sample_weight=None):
        """Behind the forward and loss at w: this rank's own gradient (no collective: under a
        process group the perturbation is per rank, m-sharpness), the perturbation, and the forward
        and loss at w + e with the same dropout masks.  The running BatchNorm statistics and
        num_batches_tracked end as the forward at w left them: snapshot before the second forward,
        put back behind it.  Returns what the step's backward consumes."""
        eng, cfg = self.eng, self.cfg
        eng.run_backward(pl, dc, dp)
        self._sam_perturb(e, g, cfg.sam_rho, cfg.sam_adaptive)
        self.sam_steps += 1
        if self._bn_snapshot is None:
            self._bn_snapshot = (torch.empty_like(eng.bn), torch.empty_like(eng.nbt))
        eng.snapshot_bn(*self._bn_snapshot)
        controls, pred_speed, pl = eng.run_forward_ft(imgs, speeds, cmds, e, g, cfg.dropout, seed)
        eng.put_back_bn(*self._bn_snapshot)
        _, dc, dp = self.loss(controls, tgts, pred_speed, speeds, out=self.sam_loss_buf,
                              sample_weight=sample_weight)
        return pl, dc, dp

    def sam_norm(self):
        """{S, norm, scale} of the last perturbation (a SAM step's or sharpness()'s) as a CPU
        float64 tensor [3]: the sum of squares, its root -- the gradient norm (ASAM: of |w| g) --
        and rho / (norm + 1e-12).  Like trust_ratios() the read is the only synchronisation."""
        if self._sam_out3 is None:
            raise RuntimeError("no SAM perturbation yet (TrainConfig.sam_rho, Trainer.sharpness)")
        return self._sam_out3.detach().cpu().clone()

    @torch.no_grad()
    def sharpness(self, batches, rho=None, adaptive=None):
        """Mean over `batches` of L(w + e(w)) - L(w), the first-order worst-case loss increase
        within rho (the quantity SAM minimises), on the kernels of the SAM step.  Per batch:
        run_forward_frozen (eval-mode BatchNorm, no dropout, buffers untouched), loss, backward,
        perturb, run_forward_frozen, loss, restore; the sums are kept on the device in float64 and
        read once at the end.  rho / adaptive: default to the config's.  OVERWRITES the gradient
        arena; parameters, moments, EMA, step counts and BatchNorm buffers are bit for bit what
        they were.  Over the trainable range when a prefix is frozen.  Allowed inside
        ``with trainer.ema_weights():`` (the averaged weights' sharpness).  Returns loss,
        loss_perturbed, sharpness, grad_norm (mean norm of sam_norm()) and batches."""
        eng = self._ensure_engine()
        rho = check_sam_rho(self.cfg.sam_rho if rho is None else rho)
        adaptive = bool(self.cfg.sam_adaptive if adaptive is None else adaptive)
        e, g = self._freeze_state()
        self._sam_buffers()
        acc = torch.zeros(3, dtype=torch.float64, device=eng.device)
        n = 0
        for imgs, speeds, cmds, tgts in batches:
            controls, pred_speed, pl = eng.run_forward_frozen(imgs, speeds, cmds)
            buf, dc, dp = self.loss(controls, tgts, pred_speed, speeds, out=self.sam_loss_buf)
            acc[0:1] += buf[0:1].double()
            eng.run_backward(pl, dc, dp)
            self._sam_perturb(e, g, rho, adaptive)
            controls, pred_speed, pl = eng.run_forward_frozen(imgs, speeds, cmds)
            buf, _, _ = self.loss(controls, tgts, pred_speed, speeds, want_grads=False,
                                  out=self.sam_loss_buf)
            acc[1:2] += buf[0:1].double()
            acc[2:3] += self._sam_out3[1:2]
            self._sam_restore(e, g)
            n += 1
        if n == 0:
            raise ValueError("Trainer.sharpness: no batches")
        a, b, c = (acc / n).tolist()
        eng.check_status()
        return {"loss": a, "loss_perturbed": b, "sharpness": b - a, "grad_norm": c, "batches": n}

    def _adam_range(self, begin, end, grad_scale, clip_ptr=None, frozen_groups=0):
        """cilrs_adam_step over the trainable part of the arena range [begin, end) (step counts
        already advanced).  Adjacent parameter groups that share learning rate and step
        count form one run; one run is the plain cilrs_adam_step launch, several (lr_mult, or
        an earlier freeze that tells the groups' step counts apart) go to the table-driven
        launch.  With EMA on, each of the two is followed by cilrs_ema_update over the same
        range, or (ema_fused) replaced by its form with the average fused in (cilrs_adam_step_ema /
        _groups_ema); this step's weight on every range."""
        eng, cfg = self.eng, self.cfg
        steps = self.group_steps
        lr_now = self.lr_now                  # == self.lr with the warm-up off or over
        runs = []                             # [begin, end, lr, step]
        for i in range(frozen_groups, 6):
            b, e = eng.group_ranges[i]
            b, e = max(b, begin), min(e, end)
            if b >= e:
                continue
            lr = lr_now * self.lr_mult[i]
            if runs and runs[-1][1] == b and runs[-1][2] == lr and runs[-1][3] == steps[i]:
                runs[-1][1] = e
            else:
                runs.append([b, e, lr, steps[i]])
        if not runs:
            return
        b, e = runs[0][0], runs[-1][1]
        if cfg.optimizer != "adam":
            self._optim_runs(runs, grad_scale, clip_ptr)
            if self.ema is not None:
                self._ema_pass(b, e)
            return
        fused_ema = self.ema is not None and self.ema_fused
        if len(runs) == 1:
            _, _, lr, step = runs[0]
            if fused_ema:
                L.check(L.lib().cilrs_adam_step_ema(
                    L.ptr(eng.params[b:e]), L.ptr(eng.grads[b:e]), L.ptr(self.exp_avg[b:e]),
                    L.ptr(self.exp_avg_sq[b:e]), e - b, lr, cfg.betas[0], cfg.betas[1], cfg.eps,
                    cfg.weight_decay, step, clip_ptr, float(grad_scale), L.ptr(self.ema[b:e]),
                    self._ema_w, self._stream()))
                return
            L.check(L.lib().cilrs_adam_step(
                L.ptr(eng.params[b:e]), L.ptr(eng.grads[b:e]), L.ptr(self.exp_avg[b:e]),
                L.ptr(self.exp_avg_sq[b:e]), e - b, lr, cfg.betas[0], cfg.betas[1], cfg.eps,
                cfg.weight_decay, step, clip_ptr, float(grad_scale), self._stream()))
            if self.ema is not None:
                self._ema_pass(b, e)
            return
        # several rates / step counts: still one launch, the kernel looks them up per range
        # (range launches cost 0.044 ms per step at B=128, DESIGN.md "Fine-tuning")
        k = len(runs)
        ends = (C.c_size_t * k)(*[r[1] - b for r in runs])
        lrs = (C.c_double * k)(*[r[2] for r in runs])
        steps = (C.c_int64 * k)(*[r[3] for r in runs])
        if fused_ema:
            L.check(L.lib().cilrs_adam_step_groups_ema(
                L.ptr(eng.params[b:e]), L.ptr(eng.grads[b:e]), L.ptr(self.exp_avg[b:e]),
                L.ptr(self.exp_avg_sq[b:e]), e - b, k, ends, lrs, steps, cfg.betas[0],
                cfg.betas[1], cfg.eps, cfg.weight_decay, clip_ptr, float(grad_scale),
                L.ptr(self.ema[b:e]), self._ema_w, self._stream()))
            return
        L.check(L.lib().cilrs_adam_step_groups(
            L.ptr(eng.params[b:e]), L.ptr(eng.grads[b:e]), L.ptr(self.exp_avg[b:e]),
            L.ptr(self.exp_avg_sq[b:e]), e - b, k, ends, lrs, steps, cfg.betas[0], cfg.betas[1],
            cfg.eps, cfg.weight_decay, clip_ptr, float(grad_scale), self._stream()))
        if self.ema is not None:
            self._ema_pass(b, e)

    def _optim_runs(self, runs, grad_scale, clip_ptr):
        """AdamW / LAMB over adjacent runs [begin, end, lr, step] of whole parameter tensors: one
        cilrs_optim_step over their segments, the runs as its groups."""
        eng, cfg = self.eng, self.cfg
        b, e = runs[0][0], runs[-1][1]
        try:
            first = self._seg_index_of_start[b]
            last = self._seg_index_of_end[e]
            for r in runs:
                self._seg_index_of_end[r[1]]
        except KeyError:
            raise RuntimeError(f"optimizer range [{b}, {e}) does not consist of whole parameter "
                               "tensors") from None
        k = len(runs)
        ends = (C.c_size_t * k)(*[r[1] for r in runs])
        lrs = (C.c_double * k)(*[r[2] for r in runs])
        steps = (C.c_int64 * k)(*[r[3] for r in runs])
        lamb = cfg.optimizer == "lamb"
        L.check(L.lib().cilrs_optim_step(
            OPTIM_KIND[cfg.optimizer], self._optim_table, first, last - first + 1,
            L.ptr(eng.params), L.ptr(eng.grads), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), k,
            ends, lrs, steps, cfg.betas[0], cfg.betas[1], cfg.eps, cfg.weight_decay,
            float(cfg.trust_clip), clip_ptr, float(grad_scale),
            L.ptr(self._optim_scratch) if lamb else None, L.ptr(self._ratios) if lamb else None,
            self._stream()))

    # -- EMA of the weights ------------------------------------------------------------------------
    def _need_ema(self):
        if self.ema is None:
            raise RuntimeError("this Trainer keeps no EMA of the weights (TrainConfig.ema_decay)")

    def ema_reset(self):
        """The average starts over: a copy of the parameters as they are now, no updates made."""
        self._need_ema()
        self._refuse_inside_ema_weights("ema_reset")
        self.ema.copy_(self.eng.params)
        self.ema_updates = 0

    def ema_state_dict(self):
        """The averaged parameters, keyed and shaped like ``model.state_dict()``'s parameter
        entries (CPU clones).  BatchNorm buffers are not averaged and not in it."""
        self._need_ema()
        from .engine import _arena_view
        src = self.eng.params if self._in_ema else self.ema    # swapped inside ema_weights()
        return {name: _arena_view(src, off, numel, shape).detach().cpu().contiguous().clone()
                for name, off, numel, shape in self.eng.params_layout}

    def load_ema_state_dict(self, sd):
        """Inverse of ema_state_dict (the update count is `ema_updates`, set by the caller)."""
        self._need_ema()
        self._refuse_inside_ema_weights("load_ema_state_dict")
        from .engine import _arena_view
        want = [p[0] for p in self.eng.params_layout]
        missing, extra = [k for k in want if k not in sd], [k for k in sd if k not in set(want)]
        if missing or extra:
            raise KeyError(f"ema_state_dict: missing {missing[:3]}, unexpected {extra[:3]}")
        with torch.no_grad():
            for name, off, numel, shape in self.eng.params_layout:
                if tuple(sd[name].shape) != tuple(shape):
                    raise ValueError(f"ema_state_dict: {name} has shape {tuple(sd[name].shape)}, "
                                     f"expected {tuple(shape)}")
                _arena_view(self.ema, off, numel, shape).copy_(sd[name])

    def _swap_ema(self):
        # Predictor and the inference lanes run on streams of their own: the exchange is fenced
        # against the whole device on both sides (it happens once per validation, not per step)
        dev = self.eng.device
        torch.cuda.synchronize(dev)
        L.check(L.lib().cilrs_swap(L.ptr(self.eng.params), L.ptr(self.ema), self.eng.n_arena,
                                   self._stream()))
        if self.ema_bn is not None:           # the averaged weights' own BatchNorm buffers
            L.check(L.lib().cilrs_swap(L.ptr(self.eng.bn), L.ptr(self.ema_bn), self.eng.bn.numel(),
                                       self._stream()))
            with torch.no_grad():
                live = self.eng.nbt.clone()
                self.eng.nbt.copy_(self.ema_nbt)
                self.ema_nbt.copy_(live)
        torch.cuda.synchronize(dev)
        self.model.weights_changed()

    @contextlib.contextmanager
    def ema_weights(self):
        """``with trainer.ema_weights():`` -- the model IS the averaged model inside: the averaged
        parameters are swapped into the arena (cilrs_swap; the plans keep their pointers) and the
        weights epoch is bumped, so ``model(...)``, Predictor and evaluate.py work unchanged, with
        the live BatchNorm buffers.  On exit, also on an exception, the raw parameters are swapped
        back.  No train_step / optimizer_step inside; not re-entrant."""
        self._need_ema()
        self._ensure_engine()
        if self._in_ema:
            raise RuntimeError("Trainer.ema_weights() is not re-entrant")
        self._swap_ema()
        self._in_ema = True
        try:
            yield self
        finally:
            try:
                self._swap_ema()
            finally:
                # also when the exchange back itself failed (a device error): the Trainer is not
                # left locked; the arena may then still hold the averaged weights, and the error
                # that says so propagates
                self._in_ema = False

    # -- BatchNorm re-estimation (bn_estimate.py) --------------------------------------------------
    def update_bn(self, batches, ema=False, estimator="batch_mean"):
        """Re-estimate every BatchNorm's running statistics on `batches` (image tensors, or tuples
        starting with one): ``torch.optim.swa_utils.update_bn`` for this module, and AdaBN.

        ema=False: of the live weights, into the module's buffers.  ema=True: of the averaged
        weights -- runs inside ``ema_weights()`` and leaves the result in a Trainer-owned pair
        (ema_bn / ema_nbt, created on first use as a copy of the live buffers) that every later
        ``ema_weights()`` exchanges together with the parameters; the live buffers and parameters
        are bit for bit what they were.  Data parallel: every rank passes its own shard, the
        tables are summed over the ranks (they add entry by entry) before the buffers are
        written, so all ranks end with identical buffers.  Returns the estimator."""
        from .bn_estimate import BatchNormEstimator
        self._ensure_engine()
        if not ema:
            self._refuse_inside_ema_weights("update_bn")
            return self._update_bn(BatchNormEstimator(self.model, estimator), batches)
        self._need_ema()
        est = BatchNormEstimator(self.model, estimator)       # (raises before anything is created)
        if self.ema_bn is None:
            self.ema_bn = self.eng.bn.clone()
            self.ema_nbt = self.eng.nbt.clone()
        with self.ema_weights():
            return self._update_bn(est, batches)

    @torch.no_grad()
    def _update_bn(self, est, batches):
        for b in batches:
            est.update(b)
        est.table = self.all_reduce_sum(est.table)
        if self.reducer is not None:
            est.batches = max(est.batches, 1)         # a rank without a batch still writes the sum
        est.finalize()
        return est

    def ema_bn_state_dict(self):
        """The averaged weights' BatchNorm buffers (update_bn(ema=True)), keyed like the model's
        buffer entries (CPU clones); None before the first such call."""
        self._need_ema()
        if self.ema_bn is None:
            return None
        bn, nbt = (self.eng.bn, self.eng.nbt) if self._in_ema else (self.ema_bn, self.ema_nbt)
        out = {}
        for j, (prefix, ch, rm, rv) in enumerate(self.eng.bn_layout):
            out[f"{prefix}.running_mean"] = bn[rm:rm + ch].detach().cpu().clone()
            out[f"{prefix}.running_var"] = bn[rv:rv + ch].detach().cpu().clone()
            out[f"{prefix}.num_batches_tracked"] = nbt[j].detach().cpu().clone()
        return out

    def load_ema_bn_state_dict(self, sd):
        """Inverse of ema_bn_state_dict."""
        self._need_ema()
        self._refuse_inside_ema_weights("load_ema_bn_state_dict")
        want = [f"{p}.{k}" for p, *_ in self.eng.bn_layout
                for k in ("running_mean", "running_var", "num_batches_tracked")]
        missing, extra = [k for k in want if k not in sd], [k for k in sd if k not in set(want)]
        if missing or extra:
            raise KeyError(f"ema_bn_state_dict: missing {missing[:3]}, unexpected {extra[:3]}")
        bn, nbt = self.eng.bn.clone(), self.eng.nbt.clone()
        with torch.no_grad():
            for j, (prefix, ch, rm, rv) in enumerate(self.eng.bn_layout):
                for key, off in (("running_mean", rm), ("running_var", rv)):
                    t = sd[f"{prefix}.{key}"]
                    if tuple(t.shape) != (ch,):
                        raise ValueError(f"ema_bn_state_dict: {prefix}.{key} has shape "
                                         f"{tuple(t.shape)}, expected {(ch,)}")
                    bn[off:off + ch].copy_(t)
                nbt[j].copy_(sd[f"{prefix}.num_batches_tracked"])
        self.ema_bn, self.ema_nbt = bn, nbt

    def next_dropout_seed(self):
        """Seed of the next train step's dropout masks: torch's seed, the step count and the
        data-parallel rank (replicas must not drop the same units)."""
        self._seed_calls += 1
        return dropout_seed(torch.initial_seed(), self._seed_calls, self.rank)

    def losses(self, check=True):
        """Host dict of the last step's loss terms (one device->host copy).  With check=True this
        synchronisation point also surfaces what the reference would have raised or shown during
        the step: an out-of-range command (torch.gather, autonomous_drive.py:397-398) and a
        non-finite loss (the reference prints NaN from its per-step .item(), nb:523-526)."""
        v = self.loss_buf[:6].tolist()
        out = dict(zip(LOSS_KEYS, v))
        if check:
            self.eng.check_status()
            if not all(x == x and abs(x) != float("inf") for x in v):
                raise FloatingPointError(f"non-finite loss after step {self.step_count}: {out}")
        return out

    def grad_norm(self):
        return float(self.clip_out[0])

    # -- StepLR (nb:535-536, 604) ----------------------------------------------------------------
    def scheduler_step(self):
        self.epoch += 1
        self.lr = scheduled_lr(self.cfg, self.epoch)

    # -- validate() (nb:563-585) -------------------------------------------------------------------
    def validate(self, batches, ema=False):
        """mean of batch means + per-command mean |steer error|, like the reference.  ema=True:
        of the averaged weights (inside ``ema_weights()``)."""
        if ema:
            with self.ema_weights():
                return self._validate(batches)
        return self._validate(batches)

    @torch.no_grad()
    def _validate(self, batches):
        self.model.eval()
        sums = torch.zeros(6, dtype=torch.float64)
        # (the reference's validate is written for its four commands, nb:566; a model built with more
        #  branches gets one row per command, named cmd<i> beyond the reference's four names)
        nc = max(4, int(getattr(self.model, "num_commands", 4)))
        cmd_sum = torch.zeros(nc, dtype=torch.float64, device=self.eng.device)
        cmd_cnt = torch.zeros(nc, dtype=torch.float64, device=self.eng.device)
        n = 0
        for imgs, speeds, cmds, tgts in batches:
            pc, ps = self.model(imgs, speeds, cmds)
            buf, _, _ = self.loss(pc, tgts, ps, speeds, want_grads=False)
            sums += buf[:6].double().cpu()
            self.eng.check_status()
            n += 1
            serr = (pc[:, 0] - tgts[:, 0]).abs().double()
            cmd_sum.index_add_(0, cmds, serr)
            cmd_cnt.index_add_(0, cmds, torch.ones_like(serr))
        # data parallel: every rank validates its own shard; the SUMS are all-reduced so that all
        # ranks see the same metrics and take the same early-stopping / checkpoint decisions (a
        # rank that stopped alone would leave the others hanging in the next gradient all-reduce)
        packed = torch.cat([sums.to(self.eng.device), torch.tensor([float(n)], dtype=torch.float64,
                                                                  device=self.eng.device),
                            cmd_sum, cmd_cnt])
        packed = self.all_reduce_sum(packed)
        sums, n = packed[:6].cpu(), float(packed[6])
        cs, cc = packed[7:7 + nc].cpu(), packed[7 + nc:7 + 2 * nc].cpu()
        out = {k: float(sums[i]) / max(n, 1.0) for i, k in enumerate(LOSS_KEYS)}
        names = [CMD_NAMES.get(i, f"cmd{i}") for i in range(nc)]
        cmd_avg = {names[i]: (float(cs[i] / cc[i]) if cc[i] > 0 else float("nan"))
                   for i in range(nc)}
        return out, cmd_avg

    @torch.no_grad()
    def row_losses(self, batches):
        """Eval-mode per-sample losses (include/cilrs_hip.h "prioritised sampling", l_b) of every
        sample of `batches`, in order, as one device fp32 tensor: what warm-starts a
        `PrioritySampler` (`sampler.update(pos, losses)`) and the per-frame error list a
        `FramePool` takes.  No gradients, no optimizer state touched."""
        self.model.eval()
        out = []
        for imgs, speeds, cmds, tgts in batches:
            pc, ps = self.model(imgs, speeds, cmds)
            rl = torch.empty(pc.size(0), dtype=torch.float32, device=pc.device)
            self.loss(pc, tgts, ps, speeds, want_grads=False, out=self.sam_loss_buf, row_loss=rl)
            out.append(rl)
        if not out:
            raise ValueError("Trainer.row_losses: no batches")
        self.eng.check_status()
        return torch.cat(out)

    def all_reduce_sum(self, t):
        """Sum of a (device) tensor over the data-parallel ranks; the tensor itself without them."""
        if self.reducer is None:
            return t
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.reducer.pg)
        return t
