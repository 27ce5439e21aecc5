"""BatchNorm re-estimation in float64 -- the definition the device table and its finalise launch are
tested against (include/cilrs_hip.h "BatchNorm re-estimation"), written on the CPU oracle.

Per BatchNorm layer and batch b, from the layer's own input x_b ([N,C,H,W], M_b = N*H*W rows):
    mean_b = mean of x_b per channel,  var_b = its biased variance
and, over the batches in order, the table
    t = number of batches,  rows = sum M_b,
    s_mean = sum mean_b,  s_uvar = sum var_b * M_b / (M_b - 1),
    s_mmean = sum M_b * mean_b,  s_mex2 = sum M_b * (var_b + mean_b^2)
from which
    "batch_mean":  running_mean = s_mean / t,  running_var = s_uvar / t,  num_batches_tracked = t
    "pooled":      N = rows, m = s_mmean / N, running_mean = m,
                   running_var = (s_mex2 / N - m^2) * N / (N - 1),  num_batches_tracked = t
"""
import copy

import numpy as np
import torch
import torch.nn as nn

ROWS = ("s_mean", "s_uvar", "s_mmean", "s_mex2")


def bn_layers(model):
    """[(name, BatchNorm2d)] in module order (the names cilrs_variant_bn_info reports)."""
    return [(n, m) for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)]


def batch_stats(model, batches):
    """Train-mode forwards of a COPY of `model` (its buffers move, the caller's do not) over
    `batches` of (imgs, speeds, cmds[, ...]); returns {name: [(M, mean, biased var)] per batch}, in the
    model's dtype, from every BatchNorm's own input."""
    m = copy.deepcopy(model).train()
    out = {n: [] for n, _ in bn_layers(m)}
    hooks = []
    for name, bn in bn_layers(m):
        def pre(_mod, args, name=name):
            x = args[0]
            M = x.numel() // x.size(1)
            out[name].append((M, x.mean(dim=(0, 2, 3)).detach().clone(),
                              x.var(dim=(0, 2, 3), unbiased=False).detach().clone()))
        hooks.append(bn.register_forward_pre_hook(pre))
    with torch.no_grad():
        for b in batches:
            m(b[0], b[1], b[2])
    for h in hooks:
        h.remove()
    return out


def table_of(stats):
    """{name: {"t", "rows", "s_mean", "s_uvar", "s_mmean", "s_mex2"}} -- the chains in float64, one
    batch after the other, every term rounded on its own (numpy does not contract)."""
    table = {}
    for name, per_batch in stats.items():
        C = per_batch[0][1].numel()
        e = {"t": 0.0, "rows": 0.0, **{k: np.zeros(C, dtype=np.float64) for k in ROWS}}
        for M, mean, var in per_batch:
            mean, var, dM = mean.double().numpy(), var.double().numpy(), np.float64(M)
            e["t"] += 1.0
            e["rows"] += dM
            e["s_mean"] = e["s_mean"] + mean
            e["s_uvar"] = e["s_uvar"] + var * (dM / np.float64(M - 1))
            e["s_mmean"] = e["s_mmean"] + dM * mean
            e["s_mex2"] = e["s_mex2"] + dM * (var + mean * mean)
        table[name] = e
    return table


def finalize(table, estimator):
    """{name: (running_mean, running_var, num_batches_tracked)} in float64 (numpy)."""
    out = {}
    for name, e in table.items():
        if e["t"] < 1:
            raise ValueError(f"{name}: no batch seen")
        if estimator == "batch_mean":
            rm, rv = e["s_mean"] / e["t"], e["s_uvar"] / e["t"]
        elif estimator == "pooled":
            N = e["rows"]
            rm = e["s_mmean"] / N
            rv = (e["s_mex2"] / N - rm * rm) * (N / (N - 1.0))
        else:
            raise ValueError(estimator)
        out[name] = (rm, rv, int(e["t"]))
    return out


def reestimate(model, batches, estimator="batch_mean"):
    return finalize(table_of(batch_stats(model, batches)), estimator)


def load_buffers(model, buffers):
    """Write {name: (rm, rv, nbt)} into the BatchNorm buffers of `model` (in its dtype)."""
    with torch.no_grad():
        for name, bn in bn_layers(model):
            rm, rv, nbt = buffers[name]
            bn.running_mean.copy_(torch.as_tensor(np.asarray(rm)))
            bn.running_var.copy_(torch.as_tensor(np.asarray(rv)))
            bn.num_batches_tracked.fill_(int(nbt))
    return model


def torch_update_bn(model, batches):
    """What torch does: a copy of `model` with reset_running_stats(), momentum = None and train-mode
    forwards over `batches`; {name: (rm, rv, nbt)} as numpy float64 / int."""
    m = copy.deepcopy(model).train()
    for _n, bn in bn_layers(m):
        bn.reset_running_stats()
        bn.momentum = None
    with torch.no_grad():
        for b in batches:
            m(b[0], b[1], b[2])
    return {n: (bn.running_mean.double().numpy().copy(), bn.running_var.double().numpy().copy(),
                int(bn.num_batches_tracked)) for n, bn in bn_layers(m)}


def buffer_errors(got, ref):
    """(largest |d running_mean| / std, largest relative |d running_var|, layer of the first, smallest
    reference running_var) over every channel of every layer; std = sqrt(reference running_var)."""
    em, ev, where, vmin = 0.0, 0.0, None, float("inf")
    for name, (rm, rv, _t) in ref.items():
        g_rm, g_rv = np.asarray(got[name][0], np.float64), np.asarray(got[name][1], np.float64)
        a = float(np.max(np.abs(g_rm - rm) / np.sqrt(rv)))
        b = float(np.max(np.abs(g_rv - rv) / rv))
        if a > em:
            em, where = a, name
        ev = max(ev, b)
        vmin = min(vmin, float(rv.min()))
    return em, ev, where, vmin
