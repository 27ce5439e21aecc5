"""Monte-Carlo dropout through the heads: the definition the engine is held to (include/cilrs_hip.h,
cilrs_heads_mc), restated on the CPU -- shared by tests/test_mc_dropout_host.py and
tests/test_mc_dropout_gpu.py.  The reference has no such path; parity is pinned by this definition.

Inputs.   One frame gives pooled features v (fp32; F = 512 for the ResNet-34 trunk, 2048 for the
          ResNet-50 variant), normalised speed x, command k and the architecture code
          trunk | num_commands << 8 (NC commands).
Call.     S samples, dropout probability p in [0, 1), a 64-bit seed.
Row.      Sample s of frame b is row r = b * S + s.
Mask.     keep(site, r, c, cols) = u >= p, u the fp32 in [0, 1) from the top 24 bits of the hash of
          seed * 0x2545F4914F6CDD1D + (site << 40) + (r * cols + c), exactly as cilrs_dropout
          computes it.  A kept value is value / (1.0f - p), a dropped value 0.
Sites.    0: speed_encoder.2 (128 columns); 1 + 2k and 2 + 2k: control_branches.k.2 and .5 (256
          columns each); 2 NC + 1: speed_predictor.2 (256 columns; 9 for the reference).
Per row.  s1 = drop_0(relu(W_se0 x + b));  f = relu(W_se3 s1 + b);
          h1 = drop_{1+2k}(relu(W_k0 [v | f] + b));  h2 = drop_{2+2k}(relu(W_k3 h1 + b));
          controls = W_k5 h2 + b;
          p1 = drop_{2NC+1}(relu(W_p0 v + b));  p2 = relu(W_p3 p1 + b);  pred_speed = W_p5 p2 + b.
Branch.   Only the commanded branch is evaluated; a command outside 0..NC-1 uses branch 0.
Stats.    Per frame and output over its S stored fp32 samples: mean = (sum x_s) / S,
          std = sqrt(sum (x_s - mean)^2 / (S - 1)) (torch's default unbiased estimate; 0 for S = 1),
          both passes in double in sample order, rounded once to fp32.
p = 0.    Every sample is the eval-mode output and std is exactly 0.
"""
import copy

import numpy as np
import torch
import torch.nn as nn

import cilrs_oracle as O

M64 = (1 << 64) - 1
TOL = 2e-5                  # samples against float64: the project's gate for the heads
TOL_STATS = 1e-6            # mean / std against float64 statistics of the stored samples


def hash_u(seed, site, n):
    """u of elements 0..n-1 of a Dropout site: the top 24 bits of splitmix64's finaliser over
    seed * 0x2545F4914F6CDD1D + (site << 40) + index, as an fp32 in [0, 1)."""
    base = (int(seed) * 0x2545F4914F6CDD1D + (int(site) << 40)) & M64
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(base)
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    top = (x >> np.uint64(40)).astype(np.uint32)                     # (x >> 32) >> 8
    return top.astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep(seed, site, rows, cols, p):
    """bool [rows, cols]: element (r, c) of the site is kept"""
    return (hash_u(seed, site, rows * cols) >= np.float32(p)).reshape(rows, cols)


def sites(nc):
    """Dropout sites per head as the engine numbers them for nc commands (O.DROPOUT_SITES
    hard-codes 9 for the speed predictor: right for nc = 4 only)."""
    return {"speed_encoder": (0,), "speed_predictor": (2 * nc + 1,),
            **{f"control_branches.{k}": (1 + 2 * k, 2 + 2 * k) for k in range(nc)}}


SITE_COLS = {"speed_encoder": 128, "speed_predictor": 256}


def row_of(b, s, B, S):
    return b * S + s


def mc_samples(model, pooled, speed, command, S, p, seed, dtype=torch.float64, sites_fn=sites,
               row_fn=row_of):
    """[B, S, 4] = (steer, throttle, brake, raw predicted speed) of every sample in `dtype`.
    model: anything with the oracle's speed_encoder / control_branches / speed_predictor.
    sites_fn / row_fn: the definition's site numbering and row rule (the host tests swap in wrong
    ones to show that the gates see them)."""
    B, nc = pooled.size(0), len(model.control_branches)
    rows = B * S
    st = sites_fn(nc)
    se = copy.deepcopy(model.speed_encoder).to(dtype)
    sp = copy.deepcopy(model.speed_predictor).to(dtype)
    # the kept value is value / (1.0f - p): the divisor is the fp32 difference
    inv = 1.0 / float(np.float32(1.0) - np.float32(p))
    pick = torch.tensor([row_fn(b, s, B, S) for b in range(B) for s in range(S)])

    def mask(site, cols):
        m = torch.from_numpy(keep(seed, site, rows, cols, p))[pick]
        return m.to(dtype) * inv

    k_of = [int(c) if 0 <= int(c) < nc else 0 for c in command.tolist()]
    masks = {st["speed_encoder"][0]: mask(st["speed_encoder"][0], 128),
             st["speed_predictor"][0]: mask(st["speed_predictor"][0], 256)}
    v = pooled.to(dtype).repeat_interleave(S, 0)
    x = speed.to(dtype).repeat_interleave(S, 0).unsqueeze(1)
    out = torch.empty(rows, 4, dtype=dtype)
    with torch.no_grad():
        f = O._seq_with_masks(se, x, masks, st["speed_encoder"])
        combined = torch.cat([v, f], dim=1)
        out[:, 3] = O._seq_with_masks(sp, v, masks, st["speed_predictor"]).squeeze(1)
        for k in sorted(set(k_of)):
            sel = torch.tensor([b * S + s for b in range(B) if k_of[b] == k for s in range(S)])
            br = copy.deepcopy(model.control_branches[k]).to(dtype)
            ks = st[f"control_branches.{k}"]
            km = {site: mask(site, 256)[sel] for site in ks}
            out[sel, :3] = O._seq_with_masks(br, combined[sel], km, ks)
    return out.view(B, S, 4)


def stats64(samples, unbiased=True):
    """(mean, std) [B, 4] in float64 of fp32 samples [B, S, 4]: two passes in sample order."""
    x = samples.detach().cpu().to(torch.float32).double().numpy()
    B, S, _ = x.shape
    total = np.zeros((B, 4))
    for s in range(S):
        total += x[:, s]
    mean = total / S
    q = np.zeros((B, 4))
    for s in range(S):
        d = x[:, s] - mean
        q += d * d
    if S == 1:
        std = np.zeros((B, 4))
    else:
        std = np.sqrt(q / (S - 1 if unbiased else S))
    return torch.from_numpy(mean), torch.from_numpy(std)


def eval_outputs(model, pooled, speed, command, dtype=torch.float64):
    """[B, 4]: the oracle's eval-mode heads on pooled features (no dropout)."""
    nc = len(model.control_branches)
    with torch.no_grad():
        v = pooled.to(dtype)
        f = copy.deepcopy(model.speed_encoder).to(dtype).eval()(speed.to(dtype).unsqueeze(1))
        combined = torch.cat([v, f], dim=1)
        ps = copy.deepcopy(model.speed_predictor).to(dtype).eval()(v)
        out = torch.empty(v.size(0), 4, dtype=dtype)
        out[:, 3] = ps.squeeze(1)
        for b, c in enumerate(command.tolist()):
            k = int(c) if 0 <= int(c) < nc else 0
            br = copy.deepcopy(model.control_branches[k]).to(dtype).eval()
            out[b, :3] = br(combined[b:b + 1])[0]
    return out


class Heads(nn.Module):
    """The heads of CILRS(num_commands, dropout) on a trunk of `feat` features
    (model/autonomous_drive.py:371-387), without a trunk: what the op-level entry needs."""

    def __init__(self, num_commands=4, feat=512, dropout=0.5):
        super().__init__()
        self.num_commands, self.feat = num_commands, feat
        self.speed_encoder = nn.Sequential(
            nn.Linear(1, 128), nn.ReLU(inplace=True), nn.Dropout(dropout),
            nn.Linear(128, 128), nn.ReLU(inplace=True))
        self.control_branches = nn.ModuleList([
            nn.Sequential(
                nn.Linear(feat + 128, 256), nn.ReLU(inplace=True), nn.Dropout(dropout),
                nn.Linear(256, 256), nn.ReLU(inplace=True), nn.Dropout(dropout),
                nn.Linear(256, 3))
            for _ in range(num_commands)])
        self.speed_predictor = nn.Sequential(
            nn.Linear(feat, 256), nn.ReLU(inplace=True), nn.Dropout(dropout),
            nn.Linear(256, 256), nn.ReLU(inplace=True),
            nn.Linear(256, 1))


def build_heads(num_commands=4, feat=512, seed=0):
    """Heads with the portable weights (O.portable_state_dict over the heads' own entries)."""
    m = Heads(num_commands, feat)
    m.load_state_dict(O.portable_state_dict(m.state_dict(), seed), strict=True)
    return m


def synthetic_features(B, feat, seed=5):
    """(non-negative pooled features [B, feat] like an average of post-ReLU maps, speed [B]) fp32"""
    u = O._hash_u01(seed, 2000, B * feat).reshape(B, feat)
    v = torch.from_numpy((u * u * 2.0).astype(np.float32))
    speed = torch.from_numpy(O._hash_u01(seed, 2001, B).astype(np.float32))
    return v, speed
