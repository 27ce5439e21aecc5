"""BatchNorm re-estimation on the device: ``update_bn`` for averaged weights, and AdaBN.

Two uses, one mechanism (include/cilrs_hip.h "BatchNorm re-estimation"):

  * weight averaging (TrainConfig.ema_decay) leaves the averaged weights on the running statistics
    of the LIVE weights -- the reason ``torch.optim.swa_utils.update_bn`` exists.  That helper
    cannot serve this module: it calls ``model(x)`` with one argument, and it relies on
    ``momentum = None``, which the engine's train step does not read (its momentum is 0.1).
  * domain adaptation without labels (AdaBN): re-estimate every BatchNorm's statistics on camera
    frames of the target domain -- the reference README's "visual distribution shift" of the campus
    map -- with no steering labels at all.

``BatchNormEstimator.update`` runs the train-mode trunk on a batch (cilrs_net_forward_bn_stats: the
train step's own launches, no heads) and adds every layer's batch statistics to a float64 table on
the device, with no host synchronisation; ``finalize`` writes all running_mean / running_var /
num_batches_tracked in one launch.  The live buffers are not touched before ``finalize``.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

ESTIMATORS = ("batch_mean", "pooled")


def estimator_code(estimator) -> int:
    """0 for "batch_mean" (torch's momentum=None cumulative average of the batch statistics),
    1 for "pooled" (the moments of all rows seen)."""
    if estimator not in ESTIMATORS:
        raise ValueError(f"estimator must be one of {ESTIMATORS}, got {estimator!r}")
    return ESTIMATORS.index(estimator)


def stats_layout(variant=0):
    """[(prefix, C, head_offset, sums_offset)] of the table, in doubles, per BatchNorm layer in
    cilrs_variant_bn_info order: {t, sum M} at head_offset, four rows of C at sums_offset."""
    lib = L.lib()
    name = C.create_string_buffer(256)
    out = []
    for j in range(lib.cilrs_variant_num_bn(variant)):
        ch, rm, rv = L.i32(), L.sz(), L.sz()
        L.check(lib.cilrs_variant_bn_info(variant, j, name, 256, C.byref(ch), C.byref(rm),
                                          C.byref(rv)))
        c2, head, sums = L.i32(), L.sz(), L.sz()
        L.check(lib.cilrs_variant_bn_stats_info(variant, j, C.byref(c2), C.byref(head),
                                                C.byref(sums)))
        assert c2.value == ch.value
        out.append((name.value.decode(), ch.value, head.value, sums.value))
    return out


def _images_of(batch):
    """The image tensor of a batch: a bare tensor, or the first entry of a tuple / list such as the
    loaders' (imgs, speeds, cmds, tgts)."""
    if isinstance(batch, (tuple, list)):
        batch = batch[0]
    if not torch.is_tensor(batch):
        raise TypeError("update_bn: a batch must be an image tensor or a tuple starting with one, "
                        f"got {type(batch).__name__}")
    return batch


class BatchNormEstimator:
    """Statistics of every BatchNorm of `model` over the batches given to ``update``.

    ``estimator="batch_mean"``: running_mean / running_var become the means of the per-batch mean /
    unbiased variance, num_batches_tracked the number of batches -- what torch computes after
    ``reset_running_stats()`` with ``momentum = None``.  ``"pooled"``: the mean and unbiased variance
    of all rows seen; a short last batch weighs by its rows.

    The table is a float64 device tensor (``table``); tables of disjoint sets of batches add entry by
    entry, which is how data-parallel ranks combine theirs (Trainer.update_bn)."""

    def __init__(self, model, estimator="batch_mean"):
        self.estimator = estimator
        self._code = estimator_code(estimator)
        self.model = model
        self.eng = model.engine()
        if self.eng.train_precision != "fp32":
            raise RuntimeError("BatchNormEstimator: fp32 plans only (the bf16 training plan takes "
                               "its statistics from bf16 tensors)")
        n = L.lib().cilrs_variant_bn_stats_doubles(self.eng.variant)
        self.table = torch.zeros(n, dtype=torch.float64, device=self.eng.device)
        self.batches = 0

    def reset(self):
        """Forget every batch seen."""
        self.table.zero_()
        self.batches = 0

    def update(self, images):
        """Add one batch of float32 NCHW images (as ``model(images, ...)`` takes them).  Any batch
        size: a plan per size serves a ragged last batch.  No host synchronisation."""
        images = _images_of(images)
        eng = self.model.engine()
        if eng is not self.eng:
            raise RuntimeError("the model was moved/re-created after the estimator was built")
        eng.run_forward_bn_stats(images, self.table)
        self.batches += 1

    def finalize(self):
        """Write running_mean / running_var / num_batches_tracked of every BatchNorm2d of the
        module (the engine's arena views) from the table, in one launch, and announce the change
        (``weights_changed()``): folded 16-bit weights, the persistent launch's tables and a
        fine-tuning prefix's cached state are rebuilt on their next use."""
        if self.batches == 0:
            raise RuntimeError("BatchNormEstimator.finalize: no batch seen (update first)")
        eng = self.eng
        L.check(L.lib().cilrs_bn_stats_finalize(eng.variant, L.ptr(self.table), self._code,
                                                L.ptr(eng.bn), L.ptr(eng.nbt), eng._stream()))
        self.model.weights_changed()


@torch.no_grad()
def update_bn(model, batches, estimator="batch_mean"):
    """Re-estimate every BatchNorm's running statistics of `model` on `batches` -- the counterpart of
    ``torch.optim.swa_utils.update_bn(loader, model)`` and the AdaBN call.  `batches`: an iterable
    of image tensors [B,3,H,W] or of tuples whose first entry is one (the loaders'
    (imgs, speeds, cmds, tgts)); speeds, commands and targets are not read.  The module's
    train / eval mode is left as it is.  Returns the estimator (its ``table`` holds the sums)."""
    est = BatchNormEstimator(model, estimator)
    for b in batches:
        est.update(b)
    est.finalize()
    return est
