"""Generate tests/golden/ref_reproject.npz by EXECUTING the reference's own
``projective_transform`` (src/geom/projective_ops.py:110-139) on the CPU, in
the build container (/root/reference exists only here; the fixture travels,
the reference does not).

What runs unchanged from the reference: ``iproj``, ``actp``, ``proj`` and
``projective_transform`` -- the back-projection with frame ii's intrinsics, the
edge transform ``poses[:, jj] * poses[:, ii].inv()`` with the stereo override
where ii == jj, the action on the point map, the projection with frame jj's
intrinsics and the depth clamp, the validity mask, and the Jacobians ``Jj = Jp
Ja``, ``Ji = -Gij.adjT(Jj)``, ``Jz = Jp (Gij * Jz)``.

Stand-ins:

* ``lietorch`` -> ``tests/_lie_ref.lietorch_standin()``: the float64 numpy
  restatement of SE3 behind lietorch's surface.  lietorch itself is absent (an
  empty submodule), so the group algebra inside the recorded numbers is the
  stand-in's; it is pinned by the definitional tests of tests/test_lie_ref.py
  (matrix exponential, the reference's SE3_exp, central differences).  What
  this fixture pins is the COMPOSITION: which frame's intrinsics go where, the
  order of the product, the stereo override, the thresholds, the layout and
  sign of every Jacobian.
* ``device="cuda"`` in the reference code -> CPU through a TorchFunctionMode
  (as make_online_fixtures.py does).
* the default dtype is float64 while the reference runs, so its Python
  constants (the stereo translation -0.1, MIN_DEPTH) enter at double
  precision like the rest of the float64 inputs.

Case: 4 frames of 12 x 17 pixels with per-frame intrinsics, 8 edges of which
one has ii == jj, ``jacobian=True``, both values of ``return_depth``; some
pixels fall under each depth threshold.  The inputs are float32 values (held
as float64), so a float32 run starts from exactly the recorded numbers.

Usage:  python tests/golden/make_reproject_fixtures.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch
from torch.overrides import TorchFunctionMode

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, ".."))

import _lie_ref as lr  # noqa: E402


class CudaToCpu(TorchFunctionMode):
    def __torch_function__(self, func, types_, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        d = kwargs.get("device")
        if d is not None and str(d).startswith("cuda"):
            kwargs["device"] = "cpu"
        return func(*args, **kwargs)


def make_inputs():
    num, ht, wd = 4, 12, 17
    k = np.arange(num, dtype=np.float64)
    intrinsics = np.array([15.0, 14.5, 8.2, 5.7])[None] * (1 + 0.02 * k)[:, None]
    xi = np.concatenate([np.stack([0.07 * k, -0.02 * k * k, 0.2 * k], -1),
                         np.array([-0.04, 0.03, 0.06])[None] * k[:, None]], axis=-1)
    poses = lr.exp(xi)
    y, x = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    depth = 0.15 + 1.5 * (0.5 + 0.5 * np.sin(0.6 * x[None] + 1.1 * k[:, None, None]) * np.cos(0.4 * y[None]))
    ii = np.array([0, 1, 2, 3, 3, 0, 2, 1], np.int64)
    jj = np.array([1, 0, 2, 0, 2, 3, 1, 3], np.int64)
    # float32 values held as float64: the GPU tests feed exactly these numbers
    r = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    return dict(poses=r(poses), disps=r(1.0 / depth), intrinsics=r(intrinsics), ii=ii, jj=jj)


def main():
    sys.modules["lietorch"] = lr.lietorch_standin()
    spec = importlib.util.spec_from_file_location("ref_projective_ops",
                                                  os.path.join(REF, "src", "geom", "projective_ops.py"))
    pops = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pops)
    SE3 = sys.modules["lietorch"].SE3

    inp = make_inputs()
    out = dict(inp)
    torch.set_default_dtype(torch.float64)
    with CudaToCpu():
        for return_depth in (False, True):
            poses = SE3(torch.from_numpy(inp["poses"])[None])
            disps = torch.from_numpy(inp["disps"])[None]
            intr = torch.from_numpy(inp["intrinsics"])[None]
            ii, jj = torch.from_numpy(inp["ii"]), torch.from_numpy(inp["jj"])
            coords, valid, (Ji, Jj, Jz) = pops.projective_transform(poses, disps, intr, ii, jj, jacobian=True,
                                                                    return_depth=return_depth)
            tag = "d1" if return_depth else "d0"
            for name, t in (("coords", coords), ("valid", valid), ("Ji", Ji), ("Jj", Jj), ("Jz", Jz)):
                out[f"{tag}_{name}"] = t.double().numpy()
    v = out["d0_valid"]
    print(f"valid share {v.mean():.3f}; coords {out['d0_coords'].shape}, Ji {out['d0_Ji'].shape}")
    assert 0 < v.mean() < 1
    Z = lr.reproject(inp["poses"], inp["disps"], inp["intrinsics"], inp["ii"], inp["jj"])["Z1"]
    print(f"depth <= 0.2: {(Z <= lr.MIN_DEPTH).sum()} pixels, < 0.1: {(Z < 0.5 * lr.MIN_DEPTH).sum()}")
    assert (Z < 0.5 * lr.MIN_DEPTH).any() and ((Z >= 0.5 * lr.MIN_DEPTH) & (Z <= lr.MIN_DEPTH)).any()
    path = os.path.join(HERE, "ref_reproject.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
