"""Generate tests/golden/ref_update_operator.npz by EXECUTING the reference's
own ``UpdateModule.forward`` (src/modules/droid_net/droid_net.py:120-153) on the
CPU in float64, with its real ``ConvGRU`` (src/modules/droid_net/gru.py, loaded
by file path).  The fixture travels; the reference does not.

Stand-ins:

* ``GradientClip`` -> identity: its forward is the identity (clipping.py:21-24).
* ``torch_scatter.scatter_mean`` is not installed where the fixture is made:
  ``scatter_mean`` of make_update_heads_fixtures.py, an ``index_add_`` sum
  divided by the count, stands in for it.  THIS ONE FUNCTION IS THE
  GENERATOR'S, NOT THE REFERENCE'S.
* ``BasicEncoder``: imported by the file, never constructed by ``UpdateModule``.

Parameters and inputs are not stored.  They are drawn from a frozen
``np.random.RandomState`` stream (``tests/_encoders_ref.op_fixture_inputs``: the
parameters of the encoders, of the GRU and of the heads by the three oracles'
``make_params``, then net, inp, corr, flow), which the tests draw again.
Everything runs in float64 (no rounding point anywhere): torch's default dtype
is set to float64, so that the zeros ``forward`` makes for ``flow=None`` are
float64 as well.

Cases, edges x ht x wd: ``a`` 2 x 3 x 5 with ii = [2, 0] and a flow; ``b`` 1 x 4 x
6 with ``ii=None, flow=None`` (the motion filter's call).  Recorded per case,
float64: ``net`` [n, 128, ht, wd], ``delta`` and ``weight`` [n, ht, wd, 2], and
for ``a`` ``eta`` [G, ht, wd] (with the factor 0.01) and ``feat`` [G, 128, ht,
wd]: the input of ``upmask``, taken with a forward pre-hook.

Usage:  python tests/golden/make_update_operator_fixtures.py <reference root>
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
sys.path.insert(0, HERE)

import _encoders_ref as er  # noqa: E402
from make_update_heads_fixtures import scatter_mean  # noqa: E402


def load_reference(ref):
    here = os.path.join(ref, "src", "modules", "droid_net")
    spec = importlib.util.spec_from_file_location("ref_gru", os.path.join(here, "gru.py"))
    gru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gru)
    scatter = types.ModuleType("torch_scatter")
    scatter.scatter_mean = scatter_mean
    pkg = types.ModuleType("src.modules.droid_net")
    pkg.ConvGRU, pkg.BasicEncoder, pkg.GradientClip = gru.ConvGRU, None, torch.nn.Identity
    for name, mod in (("torch_scatter", scatter), ("src", types.ModuleType("src")),
                      ("src.modules", types.ModuleType("src.modules")), ("src.modules.droid_net", pkg)):
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("ref_droid_net", os.path.join(here, "droid_net.py"))
    net = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(net)
    return net


def main():
    ref = load_reference(sys.argv[1])
    torch.set_default_dtype(torch.float64)
    out = {}
    for tag in er.OP_CASES:
        Pe, Pg, Ph, x = er.op_fixture_inputs(tag)
        update = ref.UpdateModule().double()
        convs = {name: update.get_submodule(name) for name in Pe}
        convs.update({"gru." + name: getattr(update.gru, name) for name in Pg})
        convs.update({name: update.get_submodule(name) for name in Ph})
        params = {**Pe, **{"gru." + k: v for k, v in Pg.items()}, **Ph}
        with torch.no_grad():
            for name, conv in convs.items():
                w, b = params[name]
                assert tuple(conv.weight.shape) == w.shape, name
                conv.weight.copy_(torch.from_numpy(w.astype(np.float64)))
                conv.bias.copy_(torch.from_numpy(b.astype(np.float64)))
            taken = []
            update.agg.upmask.register_forward_pre_hook(lambda mod, args: taken.append(args[0]))
            t = {k: None if v is None else torch.from_numpy(v.astype(np.float64) if k != "ii" else v)[None]
                 for k, v in x.items()}
            res = update(t["net"], t["inp"], t["corr"], t["flow"], None if t["ii"] is None else t["ii"][0])
            assert all(r.dtype == torch.float64 for r in res) and len(res) == (3 if x["ii"] is None else 5)
            out[f"{tag}_net"], out[f"{tag}_delta"], out[f"{tag}_weight"] = (r[0].numpy() for r in res[:3])
            if x["ii"] is not None:
                out[f"{tag}_eta"], out[f"{tag}_feat"] = res[3][0].numpy(), taken.pop().numpy()
            assert not taken
    path = os.path.join(HERE, "ref_update_operator.npz")
    np.savez_compressed(path, **out)
    for k, v in out.items():
        print(f"{k:16s} {v.dtype} {v.shape}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
