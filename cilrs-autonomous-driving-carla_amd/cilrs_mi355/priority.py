"""Loss-prioritised batch sampling on the device: prioritised replay (Schaul et al. 2016) over
recorded frames.  A per-frame priority table lives in device memory, a train step's per-sample
losses update the entries of the frames it saw (`cilrs_priority_update`), and the next batch's
index is drawn from the table there (`cilrs_priority_draw`) and handed to `cilrs_batch_assemble`
as it is -- no host round trip between a step and the next batch.  include/cilrs_hip.h
"prioritised sampling" defines the arithmetic: fixed-point priorities (uint32, 2^20 = priority 1)
and uint64 sums, so a draw is an exact function of (table, seed, counter).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L

FIXED_ONE = 1 << 20
Q_MAX = (1 << 32) - 1
MAX_ENTRIES = 1 << 31
MAX_BATCH = 1024
_M64 = (1 << 64) - 1


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def check_sampler_args(n, base=None, subset=None, n_frames=None, alpha=0.6, beta=0.4, eps=1e-3):
    """ValueError for what no sampler can serve; returns (base float32 or None, subset int64 or
    None, n_frames).  Touches no device."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not (1 <= n <= MAX_ENTRIES):
        raise ValueError(f"n must be an integer in [1, 2^31], got {n!r}")
    n = int(n)
    if _number("alpha", alpha) < 0:
        raise ValueError(f"alpha must be >= 0, got {alpha!r}")
    if not (0.0 <= _number("beta", beta) <= 1.0):
        raise ValueError(f"beta must lie in [0, 1], got {beta!r}")
    if _number("eps", eps) <= 0:
        raise ValueError(f"eps must be > 0, got {eps!r}")
    if base is not None:
        base = np.ascontiguousarray(torch.as_tensor(base).detach().cpu().numpy(), dtype=np.float32)
        if base.shape != (n,):
            raise ValueError(f"base must have shape ({n},), got {base.shape}")
        if not (np.isfinite(base).all() and (base > 0).all()):
            raise ValueError("base must be finite and positive")
    if subset is not None:
        raw = torch.as_tensor(subset).detach().cpu().numpy()
        if raw.shape != (n,) or raw.dtype.kind not in "iu":
            raise ValueError(f"subset must be {n} integers, got shape {raw.shape}, dtype {raw.dtype}")
        subset = np.ascontiguousarray(raw, dtype=np.int64)
        if n_frames is None:
            raise ValueError("subset needs n_frames, the size of the dataset it indexes")
        if int(subset.min()) < 0 or int(subset.max()) >= int(n_frames):
            bad = subset[(subset < 0) | (subset >= int(n_frames))][0]
            raise ValueError(f"subset value {int(bad)} outside [0, {int(n_frames)})")
    n_frames = n if n_frames is None else int(n_frames)
    if subset is None and n_frames < n:
        raise ValueError(f"n_frames = {n_frames} below n = {n} without a subset")
    return base, subset, n_frames


class PrioritySampler:
    """A priority table over n entries on `device` and the draws from it.

    base [n] (finite, positive): a fixed factor of every entry's priority (class balance);
    subset [n]: the dataset frame of every entry (a training split), checked against n_frames
    here, once, so that a drawn index needs no per-step check; alpha: priority = base *
    (loss + eps)^alpha; beta: importance-weight exponent; stratified: one draw per equal slice of
    the total.  Every entry starts at priority base (the running maximum starts at 1).

    Arguments are checked on the host before anything is launched.  On a device that is not a
    GPU the object holds its configuration and a loaded state only: there is no CPU fallback
    for fill, draw or update."""

    def __init__(self, n, device, base=None, subset=None, n_frames=None, alpha=0.6, beta=0.4,
                 eps=1e-3, stratified=True, seed=0):
        base, subset, n_frames = check_sampler_args(n, base, subset, n_frames, alpha, beta, eps)
        self.n, self.n_frames = int(n), n_frames
        self.device = torch.device(device)
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        self.stratified = bool(stratified)
        self.seed = int(seed) & _M64
        self.counter = 0
        self._base_host, self._subset_host = base, subset
        self.q = self.pmax = self.base = self.subset = self.scratch = None
        if self.device.type == "cuda":
            self._create()

    # -- device state -----------------------------------------------------------------------------
    def _stream(self):
        return L.C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _create(self):
        dev = self.device
        nbytes = L.lib().cilrs_priority_scratch_bytes(self.n)
        if nbytes == 0:
            raise RuntimeError("cilrs_priority_scratch_bytes refused the table size")
        # uint32 bit patterns in int32 tensors
        self.q = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.pmax = torch.full((1,), FIXED_ONE, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        if self._base_host is not None:
            self.base = torch.from_numpy(self._base_host).to(dev)
        if self._subset_host is not None:
            self.subset = torch.from_numpy(self._subset_host).to(dev)
        self.fill()

    def _need_device(self, what):
        if self.q is None or self.q.device.type != "cuda":
            raise RuntimeError(f"PrioritySampler.{what}: the table lives on a GPU (no CPU fallback)")

    def fill(self):
        """Every entry back to base times the running maximum (cilrs_priority_fill)."""
        self._need_device("fill")
        L.check(L.lib().cilrs_priority_fill(L.ptr(self.q), self.n, L.ptr(self.base),
                                            L.ptr(self.pmax), self._stream()))

    def draw(self, batch):
        """(pos, index, weight) of the next batch as device tensors: table positions (int64),
        dataset frames (int64, what `DeviceDataset._launch` takes) and importance weights (fp32,
        at most 1).  Three launches, no host synchronisation; advances the draw counter."""
        self._need_device("draw")
        batch = int(batch)
        if not (1 <= batch <= MAX_BATCH):
            raise ValueError(f"batch must lie in [1, {MAX_BATCH}], got {batch}")
        dev = self.device
        pos = torch.empty(batch, dtype=torch.int64, device=dev)
        index = torch.empty(batch, dtype=torch.int64, device=dev)
        weight = torch.empty(batch, dtype=torch.float32, device=dev)
        L.check(L.lib().cilrs_priority_draw(
            L.ptr(self.q), self.n, L.ptr(self.subset), self.n_frames, self.seed,
            self.counter & _M64, batch, 1 if self.stratified else 0, self.beta, L.ptr(pos),
            L.ptr(index), L.ptr(weight), L.ptr(self.scratch), self._stream()))
        self.counter += 1
        return pos, index, weight

    def update(self, pos, row_loss):
        """The entries at `pos` (device int64 [B]) take the priorities of `row_loss` (device fp32
        [B]); where a position repeats the last one counts.  One launch."""
        self._need_device("update")
        b = pos.numel()
        if pos.dtype != torch.int64 or row_loss.dtype != torch.float32 or row_loss.numel() != b \
                or pos.device != self.q.device or row_loss.device != self.q.device:
            raise ValueError("update: pos int64 [B] and row_loss fp32 [B] on the sampler's device")
        if not (1 <= b <= MAX_BATCH):
            raise ValueError(f"update: batch must lie in [1, {MAX_BATCH}], got {b}")
        L.check(L.lib().cilrs_priority_update(
            L.ptr(self.q), self.n, L.ptr(pos.contiguous()), L.ptr(row_loss.contiguous()),
            L.ptr(self.base), self.alpha, self.eps, L.ptr(self.pmax), b, self._stream()))

    # -- readbacks (each one synchronises) ----------------------------------------------------------
    def table(self):
        """The raw table: numpy uint32 [n]."""
        if self.q is None:
            raise RuntimeError("PrioritySampler.table: no table (not on a GPU, nothing loaded)")
        return self.q.detach().cpu().numpy().view(np.uint32).copy()

    def running_max(self):
        return int(self.pmax.detach().cpu().numpy().view(np.uint32)[0])

    def priorities(self):
        """The priorities as float64 [n] (CPU): table / 2^20."""
        return torch.from_numpy(self.table().astype(np.float64) / FIXED_ONE)

    def probabilities(self):
        """The probability of every entry in an unstratified draw, float64 [n] (CPU)."""
        t = self.table().astype(np.uint64)
        return torch.from_numpy(t.astype(np.float64) / float(int(t.sum(dtype=np.uint64))))

    # -- resume -------------------------------------------------------------------------------------
    def state_dict(self):
        """Table, running maximum, draw counter and the configuration a resume checks; tensors and
        plain values only.  A run restored from it draws the batches the saved one would have."""
        return {"n": self.n, "alpha": self.alpha, "beta": self.beta, "eps": self.eps,
                "stratified": self.stratified, "seed": self.seed, "counter": int(self.counter),
                "q": None if self.q is None else self.q.detach().cpu().clone(),
                "pmax": None if self.pmax is None else self.pmax.detach().cpu().clone()}

    def load_state_dict(self, sd):
        if int(sd["n"]) != self.n:
            raise ValueError(f"sampler state is for {int(sd['n'])} entries, this one has {self.n}")
        for k in ("alpha", "beta", "eps", "stratified", "seed"):
            if sd[k] != getattr(self, k):
                raise ValueError(f"sampler state was written with {k} = {sd[k]!r}, this sampler "
                                 f"has {getattr(self, k)!r}")
        q, pmax = sd["q"], sd["pmax"]
        if q is not None:
            if q.dtype != torch.int32 or tuple(q.shape) != (self.n,) or bool((q == 0).any()):
                raise ValueError("sampler state: q must be int32 [n] (uint32 bits) without zeros")
            if self.q is None:
                self.q, self.pmax = q.clone(), pmax.clone()
            else:
                self.q.copy_(q)
                self.pmax.copy_(pmax)
        self.counter = int(sd["counter"])


class PrioritizedBatchLoader:
    """Training batches over a `DeviceDataset`, drawn by a `PrioritySampler` over `indices`.

    base = class_balanced_weights(command[indices]), so alpha = 0 samples from the reference's
    distribution (notebook:383-423), with replacement, by the device's own generator.  The
    augmentation (and weather) records are drawn per batch on the host from the streams
    `CachedBatchLoader` uses -- they do not depend on the index -- and go to the device once per
    epoch, as there.  Each batch is the draw (three launches) plus one assemble launch that reads
    the index the draw just wrote; nothing returns to the host.  Yields (img, spd, cmd, tgt);
    `last_pos` / `last_weight` are the yielded batch's table positions and importance weights, and
    `feedback(row_loss)` hands its per-sample losses to the table (`loop.train_one_epoch` does all
    three).  len() is len(indices) // (batch_size * world_size).

    Data parallel: rank r keeps a table over its own shard indices[r::world_size]; the tables are
    independent and no collective is taken.

    view= is refused: the steering rule needs the drawn sample's speed on the host."""

    def __init__(self, dataset, indices, batch_size: int, seed: int = 0, rank: int = 0,
                 world_size: int = 1, weather=None, view=None, alpha=0.6, beta=0.4, eps=1e-3,
                 stratified=True):
        from . import data as D
        if view is not None:
            raise ValueError("PrioritizedBatchLoader: view= is not served -- the steering rule "
                             "needs the drawn sample's speed on the host, and the draw stays on "
                             "the device (use CachedBatchLoader)")
        if not (0 <= rank < world_size):
            raise ValueError(f"rank {rank} outside world of {world_size}")
        if not (1 <= int(batch_size) <= MAX_BATCH):
            raise ValueError(f"batch_size must lie in [1, {MAX_BATCH}], got {batch_size}")
        self.ds, self.bs = dataset, int(batch_size)
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        self.n_total = len(idx)
        self.idx = idx[rank::world_size]
        self.rank, self.world = rank, world_size
        self.h = getattr(dataset, "h", D.IMG_HEIGHT)
        self.w = getattr(dataset, "w", D.IMG_WIDTH)
        self.rng = np.random.default_rng([seed, rank])
        self.weather = weather
        self.wrng = np.random.default_rng([seed, rank, D.WEATHER_STREAM])
        if len(self.idx) < 1:
            raise ValueError("PrioritizedBatchLoader: no indices on this rank")
        base = D.class_balanced_weights(np.asarray(dataset.command)[self.idx])
        self.sampler = PrioritySampler(
            len(self.idx), dataset.device, base=base, subset=self.idx, n_frames=len(dataset),
            alpha=alpha, beta=beta, eps=eps, stratified=stratified,
            seed=(int(seed) * 1000003 + rank) & _M64)
        self.last_pos = self.last_index = self.last_weight = None

    def __len__(self):
        return self.n_total // (self.bs * self.world)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def feedback(self, row_loss):
        """The last yielded batch's per-sample losses (device fp32 [B]) become its priorities."""
        if self.last_pos is None:
            raise RuntimeError("PrioritizedBatchLoader.feedback before the first batch")
        self.sampler.update(self.last_pos, row_loss)

    def state_dict(self):
        """The sampler's state and the positions of the host's augmentation and weather streams
        (plain values and tensors).  Taken between epochs -- an epoch's records are drawn when it
        starts -- a loader restored from it yields the batches this one would have."""
        return {"sampler": self.sampler.state_dict(), "rng": self.rng.bit_generator.state,
                "wrng": self.wrng.bit_generator.state}

    def load_state_dict(self, sd):
        self.sampler.load_state_dict(sd["sampler"])
        self.rng.bit_generator.state = sd["rng"]
        self.wrng.bit_generator.state = sd["wrng"]

    def __iter__(self):
        from . import data as D
        ds, nb, bs = self.ds, len(self), self.bs
        if not ds.filled:
            raise RuntimeError("PrioritizedBatchLoader: the dataset's cache is not filled")
        if nb == 0:
            return
        params = np.concatenate([D.draw_aug_params(self.rng, bs, self.h, self.w)
                                 for _ in range(nb)])
        D.check_params(params, self.h, self.w)
        params_dev = torch.from_numpy(params.view(np.uint8).reshape(
            nb * bs, D.AUG_DTYPE.itemsize)).pin_memory().to(ds.device, non_blocking=True)
        wp = None
        if self.weather is not None:
            weather = np.concatenate([self.weather.draw(self.wrng, bs, self.h, self.w)
                                      for _ in range(nb)])
            D.check_weather(weather, self.h, self.w)
            weather_dev = torch.from_numpy(weather.view(np.uint8).reshape(
                nb * bs, D.WEATHER_DTYPE.itemsize)).pin_memory().to(ds.device, non_blocking=True)
            wp = weather_dev.data_ptr()
        pp = params_dev.data_ptr()
        for b in range(nb):
            pos, index, weight = self.sampler.draw(bs)
            self.last_pos, self.last_index, self.last_weight = pos, index, weight
            yield ds._launch(index.data_ptr(), pp + b * bs * D.AUG_DTYPE.itemsize, bs,
                             weather_ptr=None if wp is None
                             else wp + b * bs * D.WEATHER_DTYPE.itemsize)
