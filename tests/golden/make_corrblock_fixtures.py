"""Generate tests/golden/ref_corrblock.npz by EXECUTING the reference's own
``CorrBlock.__init__`` (src/modules/droid_net/corr.py:39-55, 81-90) on the CPU,
in the build container (/root/reference exists only here; the fixture travels,
the reference does not).

What runs unchanged from the reference: ``CorrBlock.corr`` -- both maps over
4.0, ``torch.matmul`` of the transposed first map with the second, the view as
[batch, num, ht, wd, ht, wd] -- and the pyramid loop, ``avg_pool2d(kernel 2,
stride 2)`` of the volume reshaped to [batch num ht wd, 1, ht, wd].  The maps
are float16, as the tracker's autocast hands them over, so every recorded
level holds float16 values.

Stand-in: the reference module imports ``droid_backends`` at its head; this
package's drop-in answers the import and is not called by ``__init__``.

What the fixture pins: which map indexes the leading pixel pair, the 1 / 16
scale, and the floor in the pooled sizes (9 x 11 -> 4 x 5 -> 2 x 2).

Case: 2 edges, 32 channels, 9 x 11 pixels, standard normal maps rounded to
float16 (tests/_corrblock_ref.make_maps, seed 7), ``num_levels=3``: the
reference's loop pools once more after the last level it keeps, and
``avg_pool2d`` refuses the 1 x 1 plane a fourth level would leave at this size.

Usage:  python tests/golden/make_corrblock_fixtures.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "wildgs-slam-blackwell_amd", "python"))

import _corrblock_ref as CR  # noqa: E402

E, C, H, W, SEED = 2, 32, 9, 11, 7


def main():
    spec = importlib.util.spec_from_file_location("ref_corr", os.path.join(REF, "src", "modules", "droid_net",
                                                                           "corr.py"))
    corr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(corr)

    fmap1, fmap2 = CR.make_maps(E, C, H, W, SEED)
    with torch.no_grad():
        block = corr.CorrBlock(torch.from_numpy(fmap1)[None], torch.from_numpy(fmap2)[None], num_levels=3, radius=3)
    out = dict(fmap1=fmap1, fmap2=fmap2)
    for i, level in enumerate(block.corr_pyramid):
        assert level.dtype == torch.float16 and level.shape == (E, H, W, H >> i, W >> i), (level.dtype, level.shape)
        out[f"level{i}"] = level.numpy()
    path = os.path.join(HERE, "ref_corrblock.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
