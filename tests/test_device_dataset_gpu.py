"""Device-resident dataset on the GPU: `cilrs_batch_assemble` against `cilrs_augment_u8` on the
gathered frames (bit for bit, also past 4 GiB of cache), `CachedBatchLoader` against `BatchLoader`
tensor for tensor over consecutive epochs, shards and a few train steps, and the data-parallel
fill against the single-process one."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cilrs_oracle as O
from test_host import make_sessions

pytestmark = pytest.mark.gpu

H, W = 88, 200
ALL_STAGES_SEED = 16          # draw_aug_params(default_rng(16), 16): asserted in _stage_params


def _stage_params():
    from cilrs_mi355 import data as D
    p = D.draw_aug_params(np.random.default_rng(ALL_STAGES_SEED), 16)
    assert p["rbc_on"].any() and p["hsv_on"].any() and (p["noise_std255"] > 0).any()
    assert set(p["blur_k"].tolist()) >= {3, 5}
    assert set(p["nholes"].tolist()) >= {1, 2, 3}
    return p


def test_assemble_equals_augment_on_the_gathered_frames():
    from cilrs_mi355 import _lib as L
    from cilrs_mi355 import data as D
    g = torch.Generator().manual_seed(2)
    n = 37
    cache = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    speed = torch.rand(n, generator=g).cuda()
    command = torch.randint(0, 4, (n,), generator=g).cuda()
    targets = torch.rand(n, 3, generator=g).cuda()
    ds = D.DeviceDataset.from_tensors(cache, speed, command, targets)
    index = np.array([36, 5, 0, 17, 5, 36, 9, 22, 0, 1, 30, 29, 5, 12, 35, 3])
    assert len(index) == 16 and 0 in index and 36 in index and len(set(index)) < 16 \
        and (np.diff(index) < 0).any()
    p = _stage_params()
    img, spd, cmd, tgt, out8 = ds.assemble(index, p, want_u8=True)
    sel = torch.from_numpy(index).cuda()
    want_img, want8 = D.augment_u8(cache[sel], p, want_u8=True)
    assert img.shape == (16, 3, H, W) and img.stride() == want_img.stride()
    assert torch.equal(img, want_img) and torch.equal(out8, want8)
    assert torch.equal(spd, speed.index_select(0, sel))
    assert torch.equal(cmd, command.index_select(0, sel)) and cmd.dtype == torch.int64
    assert torch.equal(tgt, targets.index_select(0, sel))
    # the C entry with only the byte output asked for: label outputs and arrays may be NULL
    only8 = torch.zeros_like(out8)
    pdev = torch.from_numpy(p.view(np.uint8).reshape(16, -1)).cuda()
    rc = L.lib().cilrs_batch_assemble(
        L.ptr(cache), n, None, None, None, L.ptr(sel), L.ptr(pdev), 16, H, W, None, L.ptr(only8),
        None, None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.check(rc)
    assert torch.equal(only8, want8)


def test_assemble_addresses_a_cache_past_4_gib():
    from cilrs_mi355 import data as D
    free = torch.cuda.mem_get_info()[0]
    if free < 8 << 30:
        pytest.skip(f"needs 8 GB of free device memory for the 4.3 GB cache, {free} bytes free")
    n = 82_000
    where = [0, 40_700, 81_999]           # byte offsets below 2^31, above 2^31, above 2^32
    assert where[0] * H * W * 3 < 1 << 31 < where[1] * H * W * 3 < 1 << 32 < where[2] * H * W * 3
    cache = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(3)
    known = torch.randint(0, 256, (3, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    labels = torch.rand(n, 5, generator=g)
    for k, i in enumerate(where):
        cache[i] = known[k]
    ds = D.DeviceDataset.from_tensors(cache, labels[:, 0].contiguous().cuda(),
                                      (labels[:, 1] * 4).long().cuda(),
                                      labels[:, 2:].contiguous().cuda())
    p16 = _stage_params()
    picks = [int(np.nonzero(p16["blur_k"] == 5)[0][0]), int(np.nonzero(p16["noise_std255"] > 0)[0][0]),
             int(np.nonzero(p16["hsv_on"])[0][0])]
    p = p16[picks]
    order = [2, 0, 1]
    img, spd, cmd, tgt, out8 = ds.assemble(np.array(where)[order], p, want_u8=True)
    want_img, want8 = D.augment_u8(known[order], p, want_u8=True)
    assert torch.equal(img, want_img) and torch.equal(out8, want8)
    sel = torch.tensor(where)[order]
    assert torch.equal(spd.cpu(), labels[sel, 0]) and torch.equal(tgt.cpu(), labels[sel, 2:])
    assert torch.equal(cmd.cpu(), (labels[sel, 1] * 4).long())
    del ds, cache
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """27 frames on disk in the reference's format, their `Sessions`, the stratified split and the
    single-process device cache (chunks of 5: six staging rounds, a ragged last one)."""
    from cilrs_mi355 import data as D
    root = str(tmp_path_factory.mktemp("sessions"))
    make_sessions(root, (14, 13))
    s = D.Sessions(root)
    tr_idx, va_idx = s.split()
    ds = D.DeviceDataset(s, "cuda", workers=3, chunk_frames=5)
    return root, s, tr_idx, va_idx, ds


def _same_batches(got_loader, want_loader, epochs):
    nb = 0
    for epoch in range(epochs):
        got, want = list(got_loader), list(want_loader)
        assert len(got) == len(want) == len(got_loader) == len(want_loader)
        for bi, (g, w) in enumerate(zip(got, want)):
            assert len(g) == len(w) == 4
            for k, (a, b) in enumerate(zip(g, w)):
                assert a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride()
                assert torch.equal(a, b), (epoch, bi, k)
        nb += len(got)
    return nb


def test_fill_holds_every_decoded_frame_and_label(dataset):
    from cilrs_mi355 import data as D
    _, s, _, _, ds = dataset
    assert len(ds) == 27 and ds.filled and ds.cache.shape == (27, H, W, 3)
    want = np.stack([D.decode_jpeg(p) for p in s.paths])
    assert np.array_equal(ds.cache.cpu().numpy(), want)
    assert np.array_equal(ds.speed.cpu().numpy(), s.speed)
    assert np.array_equal(ds.command_dev.cpu().numpy(), s.command)
    assert np.array_equal(ds.targets.cpu().numpy(), s.targets)
    assert D.DeviceDataset.cache_bytes(27) <= ds.budget_bytes <= torch.cuda.mem_get_info()[1] // 2


def test_cached_loader_equals_batch_loader_end_to_end(dataset):
    from cilrs_mi355 import data as D
    _, s, tr_idx, va_idx, ds = dataset
    dev = torch.device("cuda")
    with D.BatchLoader(s, tr_idx, batch_size=4, device=dev, train=True, seed=5) as want:
        got = D.CachedBatchLoader(ds, tr_idx, batch_size=4, train=True, seed=5)
        assert _same_batches(got, want, epochs=2) == 2 * (len(tr_idx) // 4) > 0
    with D.BatchLoader(s, va_idx, batch_size=2, device=dev, train=False) as want:
        got = D.CachedBatchLoader(ds, va_idx, batch_size=2, train=False)
        assert len(got) == 3 and len(va_idx) == 5        # the last batch is partial
        assert _same_batches(got, want, epochs=2) == 6
        seen = 0
        for bi, (img, spd, cmd, tgt) in enumerate(got):
            ids = va_idx[bi * 2:(bi + 1) * 2]
            assert img.shape == (len(ids), 3, H, W)
            for k, i in enumerate(ids):       # un-augmented: == the reference's /255 + Normalize
                want_img = O.preprocess_frame(D.decode_jpeg(s.paths[i]))[0]
                assert torch.equal(img[k].cpu(), want_img)
                assert float(spd[k]) == float(s.speed[i]) and int(cmd[k]) == int(s.command[i])
                assert torch.equal(tgt[k].cpu(), torch.from_numpy(s.targets[i]))
            seen += len(ids)
        assert seen == 5


def test_cached_loader_equals_batch_loader_on_a_shard(dataset):
    from cilrs_mi355 import data as D
    _, s, tr_idx, va_idx, ds = dataset
    dev = torch.device("cuda")
    for idx, bs, train in ((tr_idx, 4, True), (va_idx, 2, False)):
        with D.BatchLoader(s, idx, bs, dev, train, seed=5, rank=1, world_size=2) as want:
            got = D.CachedBatchLoader(ds, idx, bs, train, seed=5, rank=1, world_size=2)
            assert _same_batches(got, want, epochs=2) > 0


def test_train_steps_fed_by_either_loader_are_bit_equal(dataset):
    """Identical inputs and deterministic reductions (include/cilrs_hip.h, conventions): the loss
    buffers of two models started from the same weights agree bit for bit after every step."""
    from cilrs_mi355 import CILRS, CONFIG_A, Trainer
    from cilrs_mi355 import data as D
    _, s, tr_idx, _, ds = dataset
    dev = torch.device("cuda")
    trainers = []
    for _ in range(2):
        m = CILRS(4, dropout=0.0)
        m.load_state_dict(O.portable_state_dict(m.state_dict(), 0), strict=True)
        trainers.append(Trainer(m.cuda(), CONFIG_A))
    with D.BatchLoader(s, tr_idx, 4, dev, True, seed=5) as a:
        b = D.CachedBatchLoader(ds, tr_idx, 4, True, seed=5)
        steps = 0
        for ba, bb in zip(a, b):
            la = trainers[0].train_step(*ba).clone()
            lb = trainers[1].train_step(*bb).clone()
            assert torch.isfinite(la).all() and torch.equal(la, lb), steps
            steps += 1
            if steps == 3:
                break
    assert steps == 3


def _fill_worker(rank, world, port, q, root, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from cilrs_mi355 import data as D
        torch.cuda.set_device(0)
        s = D.Sessions(root)
        ds = D.DeviceDataset(s, "cuda", workers=2, chunk_frames=4, fill=False)
        ds.fill(process_group=dist.group.WORLD)
        torch.cuda.synchronize()
        path = os.path.join(out_dir, f"cache{rank}.pt")
        torch.save({"cache": ds.cache.cpu(), "speed": ds.speed.cpu(),
                    "command": ds.command_dev.cpu(), "targets": ds.targets.cpu()}, path)
        q.put((rank, None, path))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:                                   # surface the failure in the parent
        import traceback
        q.put((rank, traceback.format_exc() + str(e), None))


def test_two_rank_fill_equals_single_process_fill(dataset, tmp_path):
    """Rank r decodes frames r, r+2, ... (14 and 13 of the 27, in chunks of 4: the last round
    carries 2 and 1); after the all-gather both hold the single-process cache byte for byte."""
    import torch.multiprocessing as mp
    root, _, _, _, ds = dataset
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 2000) + 211
    procs = [ctx.Process(target=_fill_worker, args=(r, 2, port, q, root, str(tmp_path)))
             for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(120)
    for r in res:
        assert r[1] is None, r[1]
    for r in res:
        got = torch.load(r[2], weights_only=True)
        assert torch.equal(got["cache"], ds.cache.cpu()), r[0]
        assert torch.equal(got["speed"], ds.speed.cpu())
        assert torch.equal(got["command"], ds.command_dev.cpu())
        assert torch.equal(got["targets"], ds.targets.cpu())
