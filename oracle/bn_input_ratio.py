"""Where the network's BatchNorm inputs sit on the |mean|/std axis.

BatchNorm computes the batch variance from sums of y and y*y (csrc/bn_pool.hip), whose error in the
normalised output grows with (mean/std)^2 of the channel.  This script runs the CPU oracle's
train-mode forward on the batch of tests/golden/forward_train_b8.npz (portable weights of seed 0,
synthetic batch of the seed stored in the file), hooks every BatchNorm2d layer and prints the largest
per-channel |mean|/std of its input.  The maximum over all layers is R_net; the BatchNorm edge
tests (tests/test_ops_edges_gpu.py) hold the kernels to the unchanged parity tolerances up to
2 * ceil(R_net).

    python oracle/bn_input_ratio.py
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cilrs_oracle as O  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden", "forward_train_b8.npz")


def bn_input_ratios(seed_weights: int = 0):
    """[(layer name, channels, rows, max |mean|/std, channel)] for every BatchNorm2d, in forward order."""
    g = np.load(GOLDEN)
    imgs, spds, cmds = O.synthetic_batch(int(g["batch"]), seed=int(g["seed"]))[:3]
    model = O.build_oracle(seed_weights).train()
    rows = []

    def hook(name):
        def fn(_mod, inp):
            x = inp[0].detach().double()
            xc = x.permute(1, 0, 2, 3).reshape(x.shape[1], -1)
            mean, std = xc.mean(1), xc.var(1, unbiased=False).sqrt()
            ratio = mean.abs() / std.clamp_min(1e-300)
            c = int(ratio.argmax())
            rows.append((name, xc.shape[0], xc.shape[1], float(ratio[c]), c))
        return fn

    handles = [m.register_forward_pre_hook(hook(n)) for n, m in model.named_modules()
               if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        c, s = model(imgs, spds, cmds)
    for h in handles:
        h.remove()
    # the forward hooked here is the golden one
    assert np.abs(c.numpy() - g["controls"]).max() <= 1e-5
    assert np.abs(s.numpy() - g["pred_speed"]).max() <= 1e-5
    return rows


def main():
    rows = bn_input_ratios()
    for name, ch, m, r, c in rows:
        print(f"{name:32s} C={ch:4d} M={m:6d}  max|mean|/std = {r:8.4f}  (channel {c})")
    name, _, _, r, c = max(rows, key=lambda t: t[3])
    print(f"R_net = {r:.4f} in {name} (channel {c}); ceil = {math.ceil(r)}")


if __name__ == "__main__":
    main()
