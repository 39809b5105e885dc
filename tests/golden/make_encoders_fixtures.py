"""Generate tests/golden/ref_encoders.npz by EXECUTING the reference's own
modules on the CPU in float64: ``UpdateModule().corr_encoder`` and
``UpdateModule().flow_encoder`` (src/modules/droid_net/droid_net.py:88-100), as
``UpdateModule.forward`` calls them (droid_net.py:136-137).  The fixture
travels; the reference does not.

The module is loaded by file path.  Stand-ins, none of which is executed here:
``ConvGRU`` / ``BasicEncoder`` (constructed by ``UpdateModule()``),
``GradientClip`` and ``torch_scatter`` (imported by the file).  Every operation
recorded is the reference's.

Parameters and inputs are not stored.  They are drawn from a frozen
``np.random.RandomState`` stream (``tests/_encoders_ref.fixture_inputs``: the
seed of the case, first the parameters in the order of ``_encoders_ref.NAMES``
-- weight, then bias -- then corr, then flow), which the tests draw again:
weights scaled by 1 / sqrt(K) and rounded to float16, biases 0.1 x normal
rounded to float32, corr standard normal rounded to float16, flow uniform in
[-64, 64] rounded to float16.  Everything runs in float64 (no rounding point
anywhere).

Cases, edges x ht x wd: ``a`` 2 x 3 x 5, ``b`` 1 x 6 x 18.  Recorded per case,
float64: ``corr_out`` [n, 128, ht, wd], ``flow_out`` [n, 64, ht, wd], and for the
even channels (to keep the file under 400 KB) the first layers' outputs after
their ReLU, ``corr_hidden`` and ``flow_hidden`` [n, 64, ht, wd], taken with
forward hooks on the first ReLU of each ``Sequential`` (cloned in the hook:
the ReLU is in place, and nothing later writes its result).

Usage:  python tests/golden/make_encoders_fixtures.py <reference root>
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _encoders_ref as er  # noqa: E402


class _NeverRun(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()


def load_reference(ref):
    scatter = types.ModuleType("torch_scatter")
    scatter.scatter_mean = None
    pkg = types.ModuleType("src.modules.droid_net")
    pkg.ConvGRU = pkg.BasicEncoder = pkg.GradientClip = _NeverRun
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
    out = {}
    for tag in er.FIXTURE_CASES:
        P, (corr, flow) = er.fixture_inputs(tag)
        update = ref.UpdateModule()
        encoders = {"corr": update.corr_encoder.double(), "flow": update.flow_encoder.double()}
        with torch.no_grad():
            for name in er.NAMES:
                conv = encoders[name[:4]][int(name[-1])]
                assert tuple(conv.weight.shape) == er.SHAPES[name], name
                conv.weight.copy_(torch.from_numpy(P[name][0].astype(np.float64)))
                conv.bias.copy_(torch.from_numpy(P[name][1].astype(np.float64)))
            for key, x in (("corr", corr), ("flow", flow)):
                taken = []
                hook = encoders[key][1].register_forward_hook(lambda mod, args, res: taken.append(res.clone()))
                res = encoders[key](torch.from_numpy(x.astype(np.float64)))
                hook.remove()
                assert res.dtype == torch.float64 and len(taken) == 1 and taken[0].shape[1] == er.HIDDEN
                out[f"{tag}_{key}_out"] = res.numpy()
                out[f"{tag}_{key}_hidden"] = taken[0].numpy()[:, er.FIXTURE_HIDDEN_ROWS].copy()
    path = os.path.join(HERE, "ref_encoders.npz")
    np.savez_compressed(path, **out)
    for k, v in out.items():
        print(f"{k:16s} {v.dtype} {v.shape}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
