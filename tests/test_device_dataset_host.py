"""Device-resident dataset, host side: the epoch plan of `CachedBatchLoader` is `BatchLoader`'s
(same sampler stream, same parameter stream, carried from epoch to epoch), the memory budget is
checked before anything is decoded, and a bad index never reaches a launch.  No GPU needed."""
import numpy as np
import pytest

from cilrs_mi355 import data as D


class LabelsOnly:
    """What the samplers read of a dataset: the command column (and a length)."""
    command = np.array(([0] * 50 + [1] * 27 + [2] * 14 + [3] * 9) * 3, dtype=np.int64)
    h, w = D.IMG_HEIGHT, D.IMG_WIDTH

    def __len__(self):
        return len(self.command)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_epoch_plan_is_batch_loaders(rank, world, train):
    ds = LabelsOnly()
    idx = np.arange(len(ds))[::-1][:277].copy()          # 277: ragged against 16 and 2 * 16
    bs, seed = 16, 11
    ref = D.BatchLoader(ds, idx, bs, "cpu", train=train, seed=seed, rank=rank, world_size=world)
    got = D.CachedBatchLoader(ds, idx, bs, train=train, seed=seed, rank=rank, world_size=world)
    assert len(got) == len(ref) > 0
    for epoch in range(3):                               # the streams carry over
        if epoch == 2:                                   # a plan drawn ahead is the next epoch's
            got._plan_ahead()
        want_order = ref._order()
        want_params = []
        for b in range(len(ref)):
            n = len(want_order[b * bs:(b + 1) * bs])
            want_params.append(D.draw_aug_params(ref.rng, n, ds.h, ds.w) if train
                               else D.identity_params(n))
        want_params = np.concatenate(want_params)
        order, params = got.epoch_plan()
        assert order.dtype == np.int64 and params.dtype == D.AUG_DTYPE
        assert np.array_equal(order, want_order[:len(ref) * bs]), epoch
        assert len(order) == (len(ref) * bs if train else len(idx[rank::world]))
        assert params.tobytes() == want_params.tobytes(), epoch
    if train:                                            # a second epoch is a new draw
        again, _ = got.epoch_plan()
        assert not np.array_equal(again, order)
    with pytest.raises(ValueError):
        D.CachedBatchLoader(ds, idx, bs, train=train, rank=world, world_size=world)


def test_cache_bytes_is_exact():
    # frames uint8 [n][h][w][3] + speed f32 + command i64 + targets f32 [3] per frame
    assert D.DeviceDataset.cache_bytes(1, 88, 200) == 88 * 200 * 3 + 4 + 8 + 12
    assert D.DeviceDataset.cache_bytes(176_000, 88, 200) == 176_000 * (52_800 + 24)
    assert D.DeviceDataset.cache_bytes(82_000) > 1 << 32          # stays a Python int
    assert D.DeviceDataset.cache_bytes(0, 88, 200) == 0
    assert D.DeviceDataset.cache_bytes(7, 3, 5) == 7 * (45 + 24)


def test_over_budget_raises_before_any_decode(monkeypatch):
    import cilrs_jpeg_worker
    calls = []
    monkeypatch.setattr(cilrs_jpeg_worker, "decode_chunk",
                        lambda a: calls.append(a) or np.zeros((len(a[0]), a[1], a[2], 3), np.uint8))
    ds = LabelsOnly()
    need = D.DeviceDataset.cache_bytes(len(ds), 88, 200)
    asked = []

    def free_memory(device):
        asked.append(device)
        return (2 * need - 2, 4 * need)                  # half of it is one byte short
    with pytest.raises(RuntimeError, match=rf"{need} bytes.*{need - 1} bytes.*BatchLoader"):
        D.DeviceDataset(ds, "cuda", mem_get_info=free_memory)
    assert len(asked) == 1 and calls == []
    with pytest.raises(RuntimeError, match="BatchLoader"):
        D.DeviceDataset(ds, "cuda", budget_bytes=need - 1)
    assert calls == []
    # exactly on budget passes the check (nothing is allocated or decoded with fill=False)
    ok = D.DeviceDataset(ds, "cuda", mem_get_info=lambda d: (2 * need, 4 * need), fill=False)
    assert ok.budget_bytes == need and not ok.filled and len(ok) == len(ds) and calls == []


def test_out_of_range_index_raises_on_the_host():
    ds = D.DeviceDataset(LabelsOnly(), "cuda", budget_bytes=1 << 40, fill=False)
    n = len(ds)
    for bad in ([0, n], [-1, 3], [n + 5]):
        with pytest.raises(RuntimeError, match=r"outside \[0, %d\)" % n):
            ds.assemble(np.array(bad), D.identity_params(len(bad)))
    # the loader checks its whole epoch the same way, before the first launch
    ld = D.CachedBatchLoader(ds, np.array([0, 1, n, 2]), 2, train=False)
    with pytest.raises(RuntimeError, match=r"outside \[0, %d\)" % n):
        next(iter(ld))


def test_c_entry_rejects_bad_arguments_before_any_launch():
    """B < 1 and NULL required pointers come back through cilrs_last_error(); nothing is
    dereferenced or launched, so this needs no GPU (the pointers are never used)."""
    import ctypes as C
    from cilrs_mi355 import _lib as L
    lib = L.lib()
    x = C.c_void_p(64)

    def call(cache=x, index=x, params=x, batch=4, out=x, speed=None, out_speed=None):
        return lib.cilrs_batch_assemble(cache, 10, speed, None, None, index, params, batch, 88, 200,
                                        out, None, out_speed, None, None, None)
    for kwargs, text in ((dict(batch=0), "batch must be at least 1"),
                         (dict(batch=-3), "batch must be at least 1"),
                         (dict(cache=None), "NULL argument"), (dict(index=None), "NULL argument"),
                         (dict(params=None), "NULL argument"), (dict(out=None), "NULL argument"),
                         (dict(out_speed=x), "needs its label array")):
        assert call(**kwargs) != 0, kwargs
        assert text in lib.cilrs_last_error().decode(), kwargs
    with pytest.raises(RuntimeError, match="batch_assemble"):
        L.check(call(batch=0))
