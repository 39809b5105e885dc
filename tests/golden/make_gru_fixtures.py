"""Generate tests/golden/ref_gru.npz by EXECUTING the reference's own ``ConvGRU``
(src/modules/droid_net/gru.py:19-48) on the CPU in float64, as the update
operator calls it (droid_net.py:117, 138): ``ConvGRU(128, 128 + 128 + 64)``,
``gru(net, inp, corr, flow)``.  The fixture travels; the reference does not.

``gru.py`` is loaded by file path; it imports nothing but torch, so there is
no stand-in: every operation recorded is the reference's.

Parameters and inputs are not stored.  They are drawn from a frozen
``np.random.RandomState`` stream (``tests/_gru_ref.fixture_inputs``: the seed of
the case, first the parameters in the order of ``_gru_ref.NAMES`` -- weight,
then bias -- then net, inp, corr, flow), which the tests draw again: 3 x 3
weights scaled by 1 / sqrt(4032) and 1 x 1 weights by 1 / sqrt(128), rounded to
float16; biases 0.1 x normal, rounded to float32; inputs standard normal rounded
to float16.  All 448 input channels are live.  Everything runs in float64 (no
rounding point anywhere).

Cases, edges x ht x wd: ``a`` 2 x 3 x 5, ``b`` 1 x 6 x 18.  Recorded per case,
float64: ``gbias`` [n, 384] (the three glo terms with the convolutions' own
biases added, taken from the module's 1 x 1 convolutions on its own glo),
``net_out`` [n, 128, ht, wd], and for the even channels (to keep the file under
400 KB) ``z`` and ``rnet`` = r * net [n, 64, ht, wd], taken with forward hooks
on ``convz`` / ``convr`` / ``convz_glo`` / ``convr_glo``.  ``net_out`` is wholly
the reference's; ``z``, ``rnet`` and ``gbias`` are put together here from the
hooked outputs of its convolutions (the sigmoid of their sum, times ``net``;
the glo output plus the convolution's own bias), since ``forward`` keeps none
of them.

Usage:  python tests/golden/make_gru_fixtures.py <reference root>
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _gru_ref as gr  # noqa: E402


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("ref_gru", os.path.join(ref, "src", "modules", "droid_net", "gru.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1])
    out = {}
    for tag in gr.FIXTURE_CASES:
        P, inputs = gr.fixture_inputs(tag)
        gru = ref.ConvGRU(128, 128 + 128 + 64).double()
        with torch.no_grad():
            for name in gr.NAMES:
                conv = getattr(gru, name)
                conv.weight.copy_(torch.from_numpy(P[name][0].astype(np.float64)))
                conv.bias.copy_(torch.from_numpy(P[name][1].astype(np.float64)))
            taken = {}
            for name in ("convz", "convr", "convq", "convz_glo", "convr_glo", "convq_glo"):
                getattr(gru, name).register_forward_hook(
                    lambda mod, args, res, name=name: taken.__setitem__(name, res))
            net, inp, corr, flow = (torch.from_numpy(t.astype(np.float64)) for t in inputs)
            net_out = gru(net, inp, corr, flow)
            n = net.shape[0]
            # conv*_glo(glo) carries conv*_glo's bias; conv*'s own bias is added here
            gbias = torch.cat([taken[k + "_glo"].view(n, 128) + getattr(gru, k).bias[None]
                               for k in ("convz", "convr", "convq")], dim=1)
            z = torch.sigmoid(taken["convz"] + taken["convz_glo"])
            rnet = torch.sigmoid(taken["convr"] + taken["convr_glo"]) * net
            assert net_out.dtype == torch.float64 and net_out.shape == net.shape
        rows = gr.FIXTURE_ZR_ROWS
        out[f"{tag}_gbias"], out[f"{tag}_net_out"] = gbias.numpy(), net_out.numpy()
        out[f"{tag}_z"], out[f"{tag}_rnet"] = z.numpy()[:, rows].copy(), rnet.numpy()[:, rows].copy()
    path = os.path.join(HERE, "ref_gru.npz")
    np.savez_compressed(path, **out)
    for k, v in out.items():
        print(f"{k:16s} {v.dtype} {v.shape}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
