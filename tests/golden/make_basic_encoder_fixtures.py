"""Generate tests/golden/ref_basic_encoder.npz by EXECUTING the reference's own
``BasicEncoder`` (src/modules/droid_net/extractor.py:75-141) on the CPU in
float64, as ``DroidNet`` constructs it (droid_net.py:159-160: ``fnet`` with
``norm_fn='instance'`` and 128 outputs, ``cnet`` with ``norm_fn='none'`` and 256).
The fixture travels; the reference does not.

The module is loaded by file path; it imports only ``torch.nn``.  Every operation
recorded is the reference's.

Parameters and images are not stored.  They are drawn from a frozen
``np.random.RandomState`` stream (``tests/_basic_encoder_ref.fixture_inputs``: the
seed of the case, first the parameters in the order of ``param_shapes`` --
weight, then bias -- then the images), which the tests draw again: weights
normal x sqrt(2 / K) rounded to float16 (the cnet head scaled down further),
biases 0.1 x normal rounded to float32, images standard normal rounded to
float16.  Everything runs in float64 (no rounding point anywhere).

Cases, norm and n x H x W: ``f`` instance 1 x 16 x 24, ``c`` none 1 x 21 x 27.
Recorded per case, float64: ``out`` (the head's output, before the caller's
tanh / relu split for ``c``) and, for the even channels (to keep the file under
400 KB), taken with forward hooks and cloned there (the ReLUs are in place):
``stem`` (conv1's output, before the norm), ``layer1``, ``layer2``, ``layer3`` (the
outputs of the three stages) and ``down2`` (the output of layer2.0.downsample:
the 1 x 1 stride-2 convolution and its norm).

Usage:  python tests/golden/make_basic_encoder_fixtures.py <reference root>
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _basic_encoder_ref as br  # noqa: E402


def load_reference(ref):
    spec = importlib.util.spec_from_file_location(
        "ref_extractor", os.path.join(ref, "src", "modules", "droid_net", "extractor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1])
    out = {}
    for tag in br.FIXTURE_CASES:
        norm, P, images = br.fixture_inputs(tag)
        net = ref.BasicEncoder(out_dim=br.OUT[norm], norm_fn=norm).double().eval()
        sd = net.state_dict()
        assert sorted(k[:-7] for k in sd if k.endswith(".weight")) == sorted(P), sorted(sd)
        with torch.no_grad():
            for name, (w, b) in P.items():
                assert tuple(sd[f"{name}.weight"].shape) == w.shape, name
                sd[f"{name}.weight"].copy_(torch.from_numpy(w.astype(np.float64)))
                sd[f"{name}.bias"].copy_(torch.from_numpy(b.astype(np.float64)))
            taken, hooks = {}, []
            for key, mod in (("stem", net.conv1), ("layer1", net.layer1), ("layer2", net.layer2),
                             ("layer3", net.layer3), ("down2", net.layer2[0].downsample)):
                hooks.append(mod.register_forward_hook(
                    lambda m, args, res, key=key: taken.__setitem__(key, res.clone())))
            res = net(torch.from_numpy(images.astype(np.float64))[None])[0]
            for h in hooks:
                h.remove()
        assert res.dtype == torch.float64 and len(taken) == 5
        out[f"{tag}_out"] = res.numpy()
        for key, t in taken.items():
            out[f"{tag}_{key}"] = t.numpy()[:, br.FIXTURE_EVEN].copy()
    path = os.path.join(HERE, "ref_basic_encoder.npz")
    np.savez_compressed(path, **out)
    for k, v in out.items():
        print(f"{k:12s} {v.dtype} {v.shape}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
