"""Feature-space novelty: is this frame's feature vector like anything the trunk produced during
training?

The reference's README names why the campus map fails ("CILRS ... replicates the behaviour seen
during training in Town01") and asks for a map-agnostic safety controller on top of the CILRS
output.  Monte-Carlo dropout (Predictor.predict_uncertain) gives that controller the spread of the
heads; every Dropout sits in the heads, so it cannot see a failure that lives in the trunk.  This
module gives the other signal: the squared Mahalanobis distance of the eval-mode pooled features to
command-conditional Gaussians with one tied covariance (Lee et al., 2018), defined in
include/cilrs_hip.h ("Feature-space novelty").

    fd = FeatureDensity(model)
    for images, speeds, commands in train_batches:      # one pass, nothing copied to the host
        fd.update(images, speeds, commands)
    fd.finalize()
    fd.calibrate(held_out_batches)                      # (images, speeds, commands) as well
    fd.save("density.pth")
    ...
    controls, pred_speed, d2 = predictor.predict_novelty(frames, kmh, commands, fd)
    if fd.percentile(d2[0]) > 99.0: ...                 # a threshold with a meaning

The moments are accumulated by a HIP kernel into a float64 table on the device, the finalising
algebra runs once on the host in float64 (numpy), the score is three small launches.  fp32 only: the
fit goes through the module's fp32 eval-mode forward.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L


def table_doubles(feat: int, nc: int) -> int:
    """n[NC] | s[NC][F] | G[F][F]: cilrs_feature_moments_doubles without the library"""
    return nc * (feat + 1) + feat * feat


def finalize_tables(table, pivot, feat, nc, shrinkage):
    """The float64 algebra between the moment table and the score tables (include/cilrs_hip.h,
    "Finalise").  table: float64 [table_doubles]; pivot: [F].  Returns (mean [NC][F] float64 -- zero
    rows for the commands that never occurred --, W [F][F] float64 lower triangular, present [NC]
    bool, N)."""
    t = np.asarray(table, dtype=np.float64)
    c = np.asarray(pivot, dtype=np.float64)
    n = t[:nc]
    s = t[nc:nc + nc * feat].reshape(nc, feat)
    low = np.tril(t[nc * (feat + 1):].reshape(feat, feat))
    G = low + np.tril(low, -1).T
    present = n > 0
    N, kp = float(n.sum()), int(present.sum())
    if N - kp <= 0:
        raise RuntimeError("FeatureDensity.finalize: needs more rows than commands that occurred "
                           f"({int(N)} rows, {kp} commands)")
    m = np.zeros((nc, feat))
    m[present] = s[present] / n[present, None]
    Sw = G - (m * n[:, None]).T @ m
    sigma = Sw / (N - kp)
    sigma = 0.5 * (sigma + sigma.T)
    sig_l = (1.0 - shrinkage) * sigma + shrinkage * (np.trace(sigma) / feat) * np.eye(feat)
    Lc = np.linalg.cholesky(sig_l)
    W = np.tril(np.linalg.solve(Lc, np.eye(feat)))
    mean = np.zeros((nc, feat))
    mean[present] = c[None, :] + m[present]
    return mean, W, present, int(round(N))


class FeatureDensity:
    """Command-conditional Gaussians with a tied, shrunk covariance over the pooled trunk features
    of ``model`` (CILRS or CILRSResNet50 on the device)."""

    def __init__(self, model, shrinkage=0.01, capacity: int = 1 << 12):
        shrinkage = float(shrinkage)
        if not 0.0 < shrinkage <= 1.0:
            raise ValueError("shrinkage must be in (0, 1]")
        self.model = model
        self.shrinkage = shrinkage
        self.F = int(model.FEATURES)
        self.NC = int(model.num_commands)
        self.device = next(model.parameters()).device
        self._capacity = int(capacity)
        self.reset()

    def reset(self):
        self.table = None                 # float64 [table_doubles] on the device
        self.pivot = None                 # float32 [F] on the device
        self.status = None                # int32 [1] on the device (op-level updates)
        self.mean = self.W = None         # float32 score tables on the device
        self.present = None               # bool [NC] (host): the commands the fit saw
        self.count = 0                    # rows of the fit, known after finalize()
        self.fit_weights_key = 0
        self.log = None                   # float32 device log of the calibration scores
        self.log_count = 0
        self._sorted = None               # host copy of the sorted log

    # ---- fit ----------------------------------------------------------------------------------
    @property
    def finalized(self) -> bool:
        return self.W is not None

    def _need_finalized(self, who):
        if not self.finalized:
            raise RuntimeError(f"FeatureDensity.{who}: call finalize() first (or load a finalised "
                               "density)")

    def _need_device(self, who):
        if self.device.type != "cuda":
            raise RuntimeError(f"FeatureDensity.{who} needs the model on an MI355X (no CPU fallback)")

    def _begin(self, first_features):
        """The first batch of a fit: its column mean is the pivot (a device op, no synchronise)."""
        if self.finalized:
            raise RuntimeError("FeatureDensity: already finalised; reset() starts a new fit")
        if self.table is None:
            self.pivot = first_features.to(torch.float32).mean(dim=0).contiguous()
            self.table = torch.zeros(table_doubles(self.F, self.NC), dtype=torch.float64,
                                     device=first_features.device)
            self.status = torch.zeros(1, dtype=torch.int32, device=first_features.device)
            eng = getattr(self.model, "_engine", None)
            self.fit_weights_key = int(eng.weights_key()) if eng is not None else 0

    def _moments_op(self, features, commands):
        """cilrs_feature_moments on rows [B, ld >= F] (the launch; host tests replace it)"""
        self._need_device("update_features")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_feature_moments(
            L.ptr(features), features.stride(0), None, 0, L.ptr(commands), features.size(0), self.F,
            self.NC, L.ptr(self.pivot), L.ptr(self.table), L.ptr(self.status), L.C.c_void_p(stream)))

    def _check_rows(self, features, commands, who):
        if features.dim() != 2 or features.dtype != torch.float32 or features.size(1) < self.F or \
                features.stride(1) != 1:
            raise RuntimeError(f"FeatureDensity.{who}: features must be float32 [B, >= {self.F}] with "
                               f"unit column stride, got {features.dtype} {tuple(features.shape)}")
        if commands.dtype != torch.int64 or tuple(commands.shape) != (features.size(0),):
            raise RuntimeError(f"FeatureDensity.{who}: commands must be int64 [{features.size(0)}]")

    def update_features(self, features, commands):
        """The op-level form: add rows of already pooled features (float32 [B, ld >= F], features
        first) and their commands (int64 [B]) to the fit."""
        self._check_rows(features, commands, "update_features")
        if features.size(0) == 0:
            return
        self._begin(features[:, :self.F])
        self._moments_op(features, commands.contiguous())

    def _forward(self, images, speeds, commands):
        """The module's fp32 eval-mode forward, as Evaluator.update runs it; returns its plan."""
        self._need_device("update")
        was_training = self.model.training
        self.model.eval()
        with torch.no_grad():
            self.model(images, speeds, commands)
        if was_training:
            self.model.train()
        return self.model.engine()

    def update(self, images, speeds, commands):
        """One batch of the training set: an eval-mode forward through the module, then one launch
        that adds its pooled features to the moment table.  Nothing is copied to the host."""
        eng = self._forward(images, speeds, commands)
        self._begin(eng.plan_features(eng.last_plan))
        eng.run_feature_moments(commands.contiguous(), self.pivot, self.table)

    def finalize(self):
        """One device-to-host copy of the table, the float64 algebra, upload of the fp32 tables."""
        if self.table is None:
            raise RuntimeError("FeatureDensity.finalize: no rows yet")
        # update() reports through the plan's status word, update_features() through this one
        eng = getattr(self.model, "_engine", None)
        if eng is not None and self.device.type == "cuda":
            eng.check_status()
        if int(self.status.item()):
            self.status.zero_()
            raise RuntimeError("FeatureDensity.finalize: a command index out of range (expected "
                               f"0..{self.NC - 1}) was seen during the fit")
        mean, W, present, n = finalize_tables(self.table.cpu().numpy(), self.pivot.cpu().numpy(),
                                              self.F, self.NC, self.shrinkage)
        self.present, self.count = present, n
        dev = self.table.device
        self.mean = torch.from_numpy(mean.astype(np.float32)).to(dev)
        self.W = torch.from_numpy(W.astype(np.float32)).to(dev)
        return self

    # ---- score --------------------------------------------------------------------------------
    def check_commands(self, commands, who="score"):
        """Raise for a command that never occurred in the fit (it has no mean)."""
        self._need_finalized(who)
        c = np.asarray(commands, dtype=np.int64).reshape(-1)
        if c.size and (c.min() < 0 or c.max() >= self.NC):
            raise RuntimeError(f"FeatureDensity.{who}: command index out of range (expected "
                               f"0..{self.NC - 1})")
        unseen = sorted(set(int(k) for k in c if not self.present[k]))
        if unseen:
            raise RuntimeError(f"FeatureDensity.{who}: command(s) {unseen} never occurred in the fit")

    def check_model(self, model, who="score"):
        """Raise when this density does not describe ``model``'s features."""
        f, nc = int(model.FEATURES), int(model.num_commands)
        if f != self.F:
            raise RuntimeError(f"FeatureDensity.{who}: fitted on {self.F} features, the model has {f}")
        if nc != self.NC:
            raise RuntimeError(f"FeatureDensity.{who}: fitted for {self.NC} commands, the model has "
                               f"{nc}")

    def _score_op(self, features, commands, d2):
        """cilrs_feature_novelty on rows [B, ld >= F] (the launches; host tests replace it)"""
        self._need_device("score_features")
        b = features.size(0)
        n = L.lib().cilrs_feature_novelty_scratch_floats(self.F, b)
        scratch = torch.empty(n, dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().cilrs_feature_novelty(
            L.ptr(features), features.stride(0), None, 0, L.ptr(commands), b, self.F, self.NC,
            L.ptr(self.mean), L.ptr(self.W), L.ptr(d2), L.ptr(scratch), n, None,
            L.C.c_void_p(stream)))

    def score_features(self, features, commands):
        """d2 (float32 [B], on the features' device) of already pooled features."""
        self._need_finalized("score_features")
        self._check_rows(features, commands, "score_features")
        self.check_commands(commands.cpu().numpy(), "score_features")
        d2 = torch.empty(features.size(0), dtype=torch.float32, device=features.device)
        if features.size(0):
            self._score_op(features, commands.contiguous(), d2)
        return d2

    # ---- whitened coordinates (cilrs_mi355.select) ---------------------------------------------
    def _origin(self):
        """the mean of the first command the fit saw: any fixed origin gives the same distances"""
        return self.mean[int(np.flatnonzero(self.present)[0])]

    def whiten(self, features):
        """(features[:, :F] - mean[k0]) @ tril(W).T as float32 [B, F] on the features' device, k0
        the first command present in the fit: squared Euclidean distances between whitened rows
        are the Mahalanobis distances of the score.  One library GEMM, run once per pool."""
        self._need_finalized("whiten")
        if features.dim() != 2 or features.dtype != torch.float32 or features.size(1) < self.F:
            raise RuntimeError(f"FeatureDensity.whiten: features must be float32 [B, >= {self.F}], "
                               f"got {features.dtype} {tuple(features.shape)}")
        return (features[:, :self.F] - self._origin()) @ torch.tril(self.W).T

    def whitened_means(self):
        """The means of the commands the fit saw, in the coordinates of ``whiten``: [K', F]."""
        self._need_finalized("whitened_means")
        rows = torch.from_numpy(np.flatnonzero(self.present)).to(self.mean.device)
        return self.whiten(self.mean.index_select(0, rows))

    # ---- calibration --------------------------------------------------------------------------
    def _log_room(self, b, device):
        if self.log is None:
            self.log = torch.empty(max(self._capacity, b), dtype=torch.float32, device=device)
        if self.log_count + b > self.log.numel():             # grow like Evaluator.err
            grown = torch.empty(max(2 * self.log.numel(), self.log_count + b), dtype=torch.float32,
                                device=device)
            grown[:self.log_count] = self.log[:self.log_count]
            self.log = grown
        return self.log[self.log_count:self.log_count + b]

    def calibrate(self, batches):
        """Forwards plus scores of held-out in-distribution frames -- batches of (images, speeds,
        commands[, ...]) -- into a device log; ``quantile`` / ``percentile`` read from it."""
        self._need_finalized("calibrate")
        for batch in batches:
            images, speeds, commands = batch[0], batch[1], batch[2]
            self.check_commands(commands.cpu().numpy(), "calibrate")
            eng = self._forward(images, speeds, commands)
            out = self._log_room(images.size(0), images.device)
            eng.run_novelty(commands.contiguous(), self.mean, self.W, d2=out, owner=self)
            self.log_count += images.size(0)
            self._sorted = None
        return self

    def calibrate_features(self, features, commands):
        """The op-level form of ``calibrate``."""
        d2 = self.score_features(features, commands)
        self._log_room(d2.numel(), d2.device).copy_(d2)
        self.log_count += d2.numel()
        self._sorted = None
        return self

    def calibration_scores(self):
        """The sorted calibration scores, float32 on the host (one copy per change of the log)."""
        if self._sorted is None:
            if self.log_count == 0:
                raise RuntimeError("FeatureDensity: no calibration scores; call calibrate() first")
            self._sorted = np.sort(self.log[:self.log_count].cpu().numpy())
        return self._sorted

    def quantile(self, q):
        """The d2 below which a fraction ``q`` (0..1) of the calibration frames fell."""
        self._need_finalized("quantile")
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError("q must be in [0, 1]")
        return float(np.quantile(self.calibration_scores().astype(np.float64), q))

    def percentile(self, d2):
        """Share (0..100) of the calibration frames whose d2 was <= ``d2``; scalar or array."""
        self._need_finalized("percentile")
        s = self.calibration_scores()
        r = 100.0 * np.searchsorted(s, np.asarray(d2, dtype=np.float32), side="right") / s.size
        return float(r) if np.ndim(r) == 0 else r

    # ---- persistence --------------------------------------------------------------------------
    def state_dict(self):
        """Plain tensors and numbers (loadable under ``weights_only``)."""
        def cpu(t):
            return None if t is None else t.detach().cpu().clone()
        cal = torch.from_numpy(self.calibration_scores().copy()) if self.log_count else \
            torch.empty(0, dtype=torch.float32)
        return {
            "F": self.F, "NC": self.NC, "shrinkage": self.shrinkage, "count": int(self.count),
            "weights_key": int(self.fit_weights_key), "finalized": bool(self.finalized),
            "table": cpu(self.table), "pivot": cpu(self.pivot), "mean": cpu(self.mean),
            "W": cpu(self.W),
            "present": None if self.present is None else torch.from_numpy(np.asarray(self.present)),
            "calibration": cal,
        }

    def load_state_dict(self, sd):
        f, nc = int(sd["F"]), int(sd["NC"])
        if f != self.F:
            raise RuntimeError(f"FeatureDensity.load_state_dict: fitted on {f} features, the model "
                               f"has {self.F}")
        if nc != self.NC:
            raise RuntimeError(f"FeatureDensity.load_state_dict: fitted for {nc} commands, the model "
                               f"has {self.NC}")
        self.reset()
        dev = self.device
        self.shrinkage = float(sd["shrinkage"])
        self.count = int(sd["count"])
        self.fit_weights_key = int(sd["weights_key"])
        if sd["table"] is not None:
            self.table = sd["table"].to(device=dev, dtype=torch.float64)
            self.pivot = sd["pivot"].to(device=dev, dtype=torch.float32)
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        if sd["finalized"]:
            self.mean = sd["mean"].to(device=dev, dtype=torch.float32).contiguous()
            self.W = sd["W"].to(device=dev, dtype=torch.float32).contiguous()
            self.present = sd["present"].numpy().astype(bool)
        cal = sd["calibration"]
        if cal.numel():
            self._log_room(cal.numel(), dev).copy_(cal.to(torch.float32))
            self.log_count = cal.numel()
        return self

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        return self.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
