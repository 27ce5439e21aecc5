"""FGSM / PGD on the network's input, on the device (csrc/adversarial.hip; include/cilrs_hip.h
"adversarial robustness" is the definition).

`Attack` is the loop that `Predictor.adversarial` and `evaluate.adversarial_sweep` share: one
iteration is the eval-mode forward that keeps its graph, `cilrs_adv_direction`, the
data-gradient-only backward, the image gradient and `cilrs_adv_step` -- five library calls on the
current stream, nothing per iteration on the host.  The adversarial train step of `Trainer` uses
the same two kernels around a train-mode pass (train.py).

Perturbation sizes are in 8-bit levels of the camera frame: eps = 2 means no byte of the returned
frame is more than 2 levels from the clean one.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .predict import IMG_MEAN, IMG_STD

GOALS = ("deviate", "error", "increase", "decrease")
# 1 / (255 * std_c): one 8-bit level in the network's input units (as cilrs_attr_finalize takes it)
CHAN_SCALE = tuple(1.0 / (255.0 * sd) for sd in IMG_STD)


def _range6():
    """The images of the bytes 0 and 255 under the preprocessing, in its fp32 operation order."""
    out = []
    for m, d in zip(IMG_MEAN, IMG_STD):
        for byte in (0.0, 255.0):
            out.append(float((np.float32(byte) / np.float32(255.0) - np.float32(m)) / np.float32(d)))
    return tuple(out)


RANGE6 = _range6()


def default_alpha(eps: float, steps: int) -> float:
    """Step size when none is given: eps for one step (FGSM), else 2.5 * eps / steps."""
    return float(eps) if int(steps) == 1 else 2.5 * float(eps) / int(steps)


def default_random_start(goal: str) -> bool:
    """True for "deviate": the gradient of |dev| at dev = 0 carries no direction."""
    return goal == "deviate"


def check_level(value, name, who="adversarial"):
    """float(value) if it is a usable size in 8-bit levels (finite, >= 0), else ValueError."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer,
                                                                     np.floating)) \
            or not math.isfinite(value) or value < 0:
        raise ValueError(f"{who}: {name} must be finite and >= 0 (8-bit levels), got {value!r}")
    return float(value)


def attack_args(eps, steps, alpha, random_start, goal, seed, who="adversarial"):
    """Host-side check of an attack's own arguments (ValueError before any launch): returns
    (eps, steps, alpha, random_start, goal, seed) with the defaults filled in."""
    if not isinstance(goal, str) or goal not in GOALS:
        raise ValueError(f"{who}: unknown goal {goal!r} (one of {GOALS})")
    eps = check_level(eps, "eps", who)
    if isinstance(steps, (bool, np.bool_)) or not isinstance(steps, (int, np.integer)) or steps < 1:
        raise ValueError(f"{who}: steps must be an integer >= 1, got {steps!r}")
    steps = int(steps)
    alpha = default_alpha(eps, steps) if alpha is None else check_level(alpha, "alpha", who)
    if random_start is None:
        random_start = default_random_start(goal)
    elif not isinstance(random_start, (bool, np.bool_)):
        raise ValueError(f"{who}: random_start must be True, False or None, got {random_start!r}")
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or \
            not 0 <= seed < 1 << 64:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^64), got {seed!r}")
    return eps, steps, alpha, bool(random_start), goal, int(seed)


class Attack:
    """The device tensors of attacks on batches of `batch` frames of `h` x `w`, and the loop."""

    def __init__(self, eng, batch, h, w):
        self.eng, self.shape = eng, (batch, h, w)
        dev = eng.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.x, self.x_adv, self.best, self.g = (torch.empty(batch, 3, h, w, **f32)
                                                 for _ in range(4))
        # [clean controls | clean pred_speed | controls of the bytes | their pred_speed | dev of the
        #  best float iterate | dev of the bytes | linf (int32)]: one block, one copy to the host
        self.out = torch.zeros(11 * batch, **f32)
        b = batch
        self.ctrl0, self.spd0 = self.out[:3 * b].view(b, 3), self.out[3 * b:4 * b]
        self.ctrl_q, self.spd_q = self.out[4 * b:7 * b].view(b, 3), self.out[7 * b:8 * b]
        self.best_dev, self.dev_u8 = self.out[8 * b:9 * b], self.out[9 * b:10 * b]
        self.linf = self.out[10 * b:].view(torch.int32)
        self.dev, self.row_dir, self.scratch_f = (torch.empty(b, **f32) for _ in range(3))
        self.minus = torch.full((b,), -1.0, **f32)
        self.improved = torch.empty(b, dtype=torch.int32, device=dev)
        self.scratch_i = torch.empty(b, dtype=torch.int32, device=dev)
        self.adv_u8 = torch.empty(b, h, w, 3, dtype=torch.uint8, device=dev)

    def clean_input(self, frames_u8, out=None):
        """The preprocessing as a tensor: cilrs_attr_samples with one sample and no noise."""
        return self.eng.run_attr_samples(frames_u8, None, 0, 1, 0, 1, 0.0, 0,
                                         out=self.x if out is None else out)

    def iterate(self, speed, cmd, dc, ds, wts, ref, k, alpha, eps, goal):
        """Iteration k (0-based) on x_adv: forward, direction, data backward, image gradient, step."""
        eng = self.eng
        c, s, pl = eng.run_forward_frozen(self.x_adv, speed, cmd)
        row_dir = improved = best = None
        if goal in ("deviate", "error"):
            eng.run_adv_direction(c, s, ref[0], ref[1], wts, k == 0, self.dev, self.best_dev,
                                  self.row_dir, self.improved)
            row_dir, improved, best = self.row_dir, self.improved, self.best
        elif goal == "decrease":
            row_dir = self.minus
        eng.run_backward(pl, dc, ds, data_only=True, segments=(0, 6))
        eng.run_input_grads(pl, self.g, None)
        eng.run_adv_step(self.x, self.x_adv, self.g, alpha, eps, CHAN_SCALE, row_dir, improved,
                         best, RANGE6)

    def run(self, frames_u8, speed, cmd, dc, ds, wts, eps, steps, alpha, random_start, goal, seed,
            targets=None, score=True):
        """The whole attack on the current stream, no host synchronisation.  frames_u8 uint8
        [B,H,W,3], speed f32 [B] (normalised), cmd i64 [B], dc [B,3] / ds [B] = the weights `wts`
        as the backward's seed, targets = (controls [B,3], pred_speed [B]) for goal="error".
        Leaves the results in self.out / self.adv_u8 (score=False: without the forward on the
        bytes; ctrl_q / spd_q / dev_u8 are then not written)."""
        eng = self.eng
        eng.run_forward_frozen_u8(frames_u8, speed, cmd, out=(self.ctrl0, self.spd0))
        clean = (self.ctrl0, self.spd0)
        ref = targets if goal == "error" else clean
        self.clean_input(frames_u8)
        eng.run_adv_start(self.x, eps if random_start else 0.0, CHAN_SCALE, seed, self.x_adv, RANGE6)
        self.best.copy_(self.x_adv)        # defined even where no iterate is ever finite
        for k in range(steps):
            self.iterate(speed, cmd, dc, ds, wts, ref, k, alpha, eps, goal)
        # fold the last iterate in: a forward, the direction, the conditional copy alone
        c, s, _ = eng.run_forward_frozen(self.x_adv, speed, cmd)
        tracked = goal in ("deviate", "error")
        eng.run_adv_direction(c, s, ref[0], ref[1], wts, not tracked, self.dev, self.best_dev,
                              self.row_dir, self.improved)
        eng.run_adv_step(self.x, self.x_adv, None, 0.0, eps, CHAN_SCALE, None, self.improved,
                         self.best)
        eng.run_adv_quantize(self.best, frames_u8, self.adv_u8, self.linf)
        if score:
            eng.run_forward_frozen_u8(self.adv_u8, speed, cmd, out=(self.ctrl_q, self.spd_q))
            eng.run_adv_direction(self.ctrl_q, self.spd_q, ref[0], ref[1], wts, True, self.dev_u8,
                                  self.scratch_f, self.row_dir, self.scratch_i)

    def random_sign_control(self, frames_u8, eps, seed):
        """The control of a sweep: one cilrs_adv_step of size eps from the clean image along a
        RANDOM sign per element (the sign of cilrs_adv_start's 2u - 1 draw, written to the gradient
        buffer), quantised into self.adv_u8 / self.linf."""
        eng = self.eng
        self.clean_input(frames_u8)
        self.x_adv.zero_()
        eng.run_adv_start(self.x_adv, 1.0, CHAN_SCALE, seed, self.g)      # g = e_c * r: r's sign
        eng.run_adv_start(self.x, 0.0, CHAN_SCALE, 0, self.x_adv)         # x_adv = x
        eng.run_adv_step(self.x, self.x_adv, self.g, eps, eps, CHAN_SCALE, None, None, None, RANGE6)
        eng.run_adv_quantize(self.x_adv, frames_u8, self.adv_u8, self.linf)
