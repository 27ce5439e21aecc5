#!/usr/bin/env python3
"""Where the cached loader's distance to a resident batch comes from (DESIGN.md section 3,
"Device-resident dataset").  ms per train step, fp32 and bf16, three rounds, alternating:
  resident              the step on one resident batch
  resident_plus_launch  the same, with one cilrs_batch_assemble launch per step (result dropped)
  trained_on_launch     the step on that launch's result (same index and parameters every step)
  resident_clone        the resident batch copied into a fresh buffer every step
  cached                fresh batches from CachedBatchLoader
The cache is 4,096 random frames made on the device's host side from a seed (no JPEGs needed)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cilrs-autonomous-driving-carla_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cilrs_mi355 import CILRS, CONFIG_A, Trainer  # noqa: E402
from cilrs_mi355 import data as D  # noqa: E402

N, B, STEPS = 4096, 128, 128


def main():
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    cache = torch.randint(0, 256, (N, 88, 200, 3), dtype=torch.uint8, generator=g).to(dev)
    ds = D.DeviceDataset.from_tensors(cache, torch.rand(N, generator=g).to(dev),
                                      torch.randint(0, 4, (N,), generator=g).to(dev),
                                      torch.rand(N, 3, generator=g).to(dev))
    cl = D.CachedBatchLoader(ds, np.arange(N), B, train=True, seed=1)
    order, params = cl.epoch_plan()
    od = torch.from_numpy(order[:B].copy()).to(dev)
    pd = torch.from_numpy(params[:B].copy().view(np.uint8).reshape(B, -1)).to(dev)
    for prec in ("fp32", "bf16"):
        tr = Trainer(CILRS(4, dropout=0.0).to(dev), CONFIG_A, precision=prec)
        res = next(iter(cl))

        def resident():
            for _ in range(STEPS):
                yield res

        def resident_plus_launch():
            for _ in range(STEPS):
                ds._launch(od.data_ptr(), pd.data_ptr(), B)
                yield res

        def trained_on_launch():
            for _ in range(STEPS):
                yield ds._launch(od.data_ptr(), pd.data_ptr(), B)

        def resident_clone():
            for _ in range(STEPS):
                yield (res[0].permute(0, 2, 3, 1).clone().permute(0, 3, 1, 2),) + tuple(res[1:])

        def cached():
            n = 0
            while n < STEPS:
                for b in cl:
                    yield b
                    n += 1
                    if n == STEPS:
                        break

        legs = {f.__name__: f for f in (resident, resident_plus_launch, trained_on_launch,
                                        resident_clone, cached)}

        def run(gen):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for b in gen():
                tr.train_step(*b)
                n += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        for f in legs.values():          # warm-up
            run(f)
        for r in range(3):
            print(prec, r, " ".join(f"{k}={run(f):.3f}ms" for k, f in legs.items()), flush=True)
        del tr


if __name__ == "__main__":
    main()
