"""Generate tests/golden/ref_update_heads.npz by EXECUTING the reference's own
modules on the CPU: ``UpdateModule().delta``, ``UpdateModule().weight`` and
``GraphAgg().forward`` (src/modules/droid_net/droid_net.py:48-80, 102-115).
The fixture travels; the reference does not.

The module is loaded by file path.  Stand-ins:

* ``ConvGRU`` / ``BasicEncoder``: constructed by ``UpdateModule()``, never
  executed.
* ``GradientClip`` -> identity: its forward is the identity (clipping.py:21-24).
* ``torch_scatter.scatter_mean`` is not installed where the fixture is made:
  ``scatter_mean`` below, an ``index_add_`` sum divided by the count (zero for
  an index without an entry), stands in for it.  THIS ONE FUNCTION IS THE
  GENERATOR'S, NOT THE REFERENCE'S; everything else ``GraphAgg.forward`` runs is
  the reference's code.

Parameters: ``torch.manual_seed(11)``, the modules' own initialisation, weights
rounded to float16 and biases to float32, everything run in float64 (no
rounding point anywhere).  To keep the file small only the first 32 input
channels of ``net`` are non-zero, and so that ``conv2`` also reads 32 live
channels the rows 32.. of ``conv1`` (weight and bias) are set to zero; the
matching weight slices are stored (``<name>_w`` [C_out, 32, 3, 3] float16 for
delta.0, weight.0, agg.conv1, agg.conv2; all 128 input channels for the
second layers and eta), ``<name>_b`` float32.

Cases, edges x ht x wd: ``a`` 5 x 3 x 5 with ii = [2, 0, 2, 5, 0], ``b`` 4 x 9 x
11 with ii = [1, 1, 1, 3].  ``net`` is standard normal rounded to float16.
Recorded per case: ``net`` [n, 32, ht, wd] float16, ``ii``, ``delta`` and
``weight`` [n, ht, wd, 2] float64 (the permuted form of droid_net.py:144-145),
``eta`` [G, ht, wd] float64 (with the factor 0.01) and ``feat`` [G, 128, ht,
wd] float64: the input of ``upmask``, taken with a forward pre-hook.

Usage:  python tests/golden/make_update_heads_fixtures.py <reference root>
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"a": (5, 3, 5, [2, 0, 2, 5, 0]), "b": (4, 9, 11, [1, 1, 1, 3])}
LIVE = 32
FIRST = ("delta.0", "weight.0", "agg.conv1", "agg.conv2")   # stored as [:, :LIVE]
SECOND = ("delta.2", "weight.2", "agg.eta.0")


def scatter_mean(src, index, dim):
    """The stand-in for torch_scatter.scatter_mean (see the module docstring)."""
    assert dim == 1
    size = int(index.max()) + 1
    out = torch.zeros(src.shape[:1] + (size,) + src.shape[2:], dtype=src.dtype)
    out.index_add_(1, index, src)
    count = torch.zeros(size, dtype=src.dtype).index_add_(0, index, torch.ones(len(index), dtype=src.dtype))
    return out / count.clamp(min=1).view(1, size, *([1] * (src.dim() - 2)))


class _NeverRun(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()


def load_reference(ref):
    scatter = types.ModuleType("torch_scatter")
    scatter.scatter_mean = scatter_mean
    pkg = types.ModuleType("src.modules.droid_net")
    pkg.ConvGRU = pkg.BasicEncoder = _NeverRun
    pkg.GradientClip = torch.nn.Identity
    for name, mod in (("torch_scatter", scatter), ("src", types.ModuleType("src")),
                      ("src.modules", types.ModuleType("src.modules")), ("src.modules.droid_net", pkg)):
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location(
        "ref_droid_net", os.path.join(ref, "src", "modules", "droid_net", "droid_net.py"))
    net = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(net)
    return net


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(20240611)
    torch.manual_seed(11)
    update = ref.UpdateModule()
    convs = {"delta.0": update.delta[0], "delta.2": update.delta[2], "weight.0": update.weight[0],
             "weight.2": update.weight[2], "agg.conv1": update.agg.conv1, "agg.conv2": update.agg.conv2,
             "agg.eta.0": update.agg.eta[0]}
    out = {}
    with torch.no_grad():
        update.agg.conv1.weight[LIVE:] = 0
        update.agg.conv1.bias[LIVE:] = 0
        for name, conv in convs.items():
            w, b = conv.weight.detach().half(), conv.bias.detach().float()
            conv.double()
            conv.weight.copy_(w.double())
            conv.bias.copy_(b.double())
            key = name.replace(".", "_")
            out[key + "_w"] = (w[:, :LIVE] if name in FIRST else w).numpy()
            out[key + "_b"] = b.numpy()
        taken = []
        update.agg.upmask.double().register_forward_pre_hook(lambda mod, args: taken.append(args[0]))
        for tag, (n, ht, wd, ii) in CASES.items():
            net16 = rng.standard_normal((n, LIVE, ht, wd)).astype(np.float16)
            net = torch.zeros(n, 128, ht, wd, dtype=torch.float64)
            net[:, :LIVE] = torch.from_numpy(net16).double()
            delta = update.delta(net).view(1, n, -1, ht, wd).permute(0, 1, 3, 4, 2)[..., :2].contiguous()[0]
            weight = update.weight(net).view(1, n, -1, ht, wd).permute(0, 1, 3, 4, 2)[..., :2].contiguous()[0]
            eta, _ = update.agg(net[None], torch.tensor(ii))
            feat = taken.pop()
            G = len(set(ii))
            assert eta.shape == (1, G, ht, wd) and feat.shape == (G, 128, ht, wd) and not taken
            assert delta.shape == weight.shape == (n, ht, wd, 2) and eta.dtype == torch.float64
            out[f"{tag}_net"], out[f"{tag}_ii"] = net16, np.asarray(ii, np.int64)
            out[f"{tag}_delta"], out[f"{tag}_weight"] = delta.numpy(), weight.numpy()
            out[f"{tag}_eta"], out[f"{tag}_feat"] = eta[0].numpy(), feat.numpy()
    path = os.path.join(HERE, "ref_update_heads.npz")
    np.savez_compressed(path, **out)
    for k, v in out.items():
        print(f"{k:16s} {v.dtype} {v.shape}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
