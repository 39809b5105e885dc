"""Generate tests/golden/ref_upsample.npz by EXECUTING the reference's own
``cvx_upsample``, ``upsample_disp`` (src/modules/droid_net/droid_net.py:23-45)
and ``GraphAgg().upmask`` (droid_net.py:61-63) on the CPU.  The fixture
travels; the reference does not.

The module is loaded by file path.  Stand-ins, none of which the recorded
functions execute: ``torch_scatter`` (``scatter_mean``, used by
``GraphAgg.forward`` only) and the ``src.modules.droid_net`` package's
``ConvGRU`` / ``BasicEncoder`` / ``GradientClip`` (``GraphAgg()`` constructs a
``GradientClip`` inside its ``eta`` head, which is not run).

Cases (n x ht x wd): ``a`` 2 x 3 x 5 (every pixel at a border) and ``b`` 1 x 9
x 11.  Masks are standard normal x 3 rounded to float16 (stored as float16),
data uniform in [0.1, 1.1] as float32 values.  Recorded per case:

* ``up1`` / ``up2``   cvx_upsample in float64 for dim 1 and 2
* ``disp_up``         upsample_disp in float64, [1, n, 8 ht, 8 wd]
* ``up1_update``      the ``FactorGraph.update`` path: the float16 mask itself
                      with autocast off and float32 data, so the softmax
                      weights are rounded to float16 (float32 result)

and for case ``a`` the head: ``GraphAgg()`` seeded, its ``upmask`` parameters
rounded to float16 (weight) / float32 (bias), run in float64 on features whose
first C = 32 channels are float16 values and whose other 96 are zero -- so the
output is exactly ``weight[:, :32] . feat + bias``: ``head_weight`` [576, 32],
``head_bias`` [576], ``head_feat`` [n, 32, ht, wd], ``head_logits`` (float64,
before any rounding) and ``head_up`` = cvx_upsample of the dim-1 data with the
logits rounded to float16, in float64.

Usage:  python tests/golden/make_upsample_fixtures.py <reference root>
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"a": (2, 3, 5), "b": (1, 9, 11)}
HEAD_C = 32


def load_reference(ref):
    scatter = types.ModuleType("torch_scatter")
    scatter.scatter_mean = None
    pkg = types.ModuleType("src.modules.droid_net")
    pkg.ConvGRU = pkg.BasicEncoder = torch.nn.Module
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
    net = load_reference(sys.argv[1])
    rng = np.random.default_rng(20240607)
    out = {}
    with torch.no_grad():
        for tag, (n, ht, wd) in CASES.items():
            mask = (3.0 * rng.standard_normal((n, 576, ht, wd))).astype(np.float16)
            data = rng.uniform(0.1, 1.1, (n, ht, wd, 2)).astype(np.float32)
            out[f"{tag}_mask"], out[f"{tag}_data"] = mask, data
            m64 = torch.from_numpy(mask).double()
            d64 = torch.from_numpy(data).double()
            out[f"{tag}_up1"] = net.cvx_upsample(d64[..., :1], m64).numpy()
            out[f"{tag}_up2"] = net.cvx_upsample(d64, m64).numpy()
            out[f"{tag}_disp_up"] = net.upsample_disp(d64[None, ..., 0], m64[None]).numpy()
            up = net.cvx_upsample(torch.from_numpy(data[..., :1]), torch.from_numpy(mask))
            assert up.dtype == torch.float32
            out[f"{tag}_up1_update"] = up.numpy()
            assert out[f"{tag}_up1"].shape == (n, 8 * ht, 8 * wd, 1) and out[f"{tag}_up2"].shape[-1] == 2
            assert out[f"{tag}_disp_up"].shape == (1, n, 8 * ht, 8 * wd)

        torch.manual_seed(7)
        conv = net.GraphAgg().upmask[0]
        assert tuple(conv.weight.shape) == (576, 128, 1, 1)
        weight = conv.weight.detach().half()
        bias = conv.bias.detach().float()
        conv = conv.double()
        conv.weight.copy_(weight.double())
        conv.bias.copy_(bias.double())
        n, ht, wd = CASES["a"]
        feat = rng.standard_normal((n, HEAD_C, ht, wd)).astype(np.float16)
        full = torch.zeros(n, 128, ht, wd, dtype=torch.float64)
        full[:, :HEAD_C] = torch.from_numpy(feat).double()
        logits = conv(full)
        out["head_weight"] = weight[:, :HEAD_C, 0, 0].numpy()
        out["head_bias"] = bias.numpy()
        out["head_feat"] = feat
        out["head_logits"] = logits.numpy()
        d64 = torch.from_numpy(out["a_data"][..., :1]).double()
        out["head_up"] = net.cvx_upsample(d64, logits.half().double()).numpy()
    path = os.path.join(HERE, "ref_upsample.npz")
    np.savez_compressed(path, **out)
    for k, v in out.items():
        print(f"{k:16s} {v.dtype} {v.shape}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
