"""Generate tests/golden/ref_mono_filter.npz by EXECUTING the reference's own
``DepthVideo.filter_high_err_mono_depth`` (src/depth_video.py:281-349) on the
CPU, in the build container (/root/reference exists only here; the fixture
travels, the reference does not).

What runs unchanged from the reference: the method itself, unbound, on a
stand-in object that carries the attributes it reads (``cfg``, ``poses``,
``mono_disps_up``, ``mono_disps_mask_up``, ``disps_up``, ``intrinsics``,
``dino_feats``, ``down_scale``, ``device``), and ``iproj`` / ``actp`` / ``proj`` of
src/geom/projective_ops.py under it.

Stand-ins:

* ``lietorch`` -> ``tests/_lie_ref.lietorch_standin()`` (as
  make_reproject_fixtures.py); the other modules depth_video.py imports and the
  method does not use (``droid_backends``, ``src.geom.ba``, ``src.modules.droid_net``,
  ``src.utils.*``) are empty modules with the imported names.
* ``device="cuda"`` -> CPU through a TorchFunctionMode; the object's ``device``
  is "cpu".
* the default dtype is float64 and ``torch.set_num_threads(1)``: the three
  ``index_put``s with duplicate indices then run in order on one thread, so
  that the last write -- the largest source index -- wins, which is the rule
  the restatement and the kernel define.

The inputs are float32 values; the reference computes on them in float64.  The
recorded mask must equal that of tests/_mono_filter_ref.py (asserted here).

Case: 58 x 75 pixels (neither a multiple of 14 nor of 8: a 4 x 5 cell map), C =
384, five frames, idx = 0 and four neighbours looking at one plane with a 1 %
ripple on the depth.  Frames 1 and 2 hold a rectangle whose depth is scaled by
0.6 and 0.7 (the moving objects: inaccurate counts); frame 0 and frame 2 hold
a block of disparity exactly 0; frame 3 stands much closer to the plane
(zoomed: its pixels fall many-to-one into a part of frame 0, the collisions);
frame 4 stands behind frame 0 and holds a rectangle of very small depth whose
points come out with Z < 0.1 and, Z replaced by 1, land inside the image.  The
DINO maps are a smooth low-rank field of the world point a cell sees plus
noise, sized so that a good half of the valid candidates match.

Usage:  python tests/golden/make_mono_filter_fixtures.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch.overrides import TorchFunctionMode

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, ".."))

import _lie_ref as lr  # noqa: E402
import _mono_filter_ref as mf  # noqa: E402

H, W, C = 58, 75, 384
IDX, JJ = 0, [1, 2, 3, 4]
NOISE = 0.55  # of the DINO maps, against a field of unit amplitude


class CudaToCpu(TorchFunctionMode):
    def __torch_function__(self, func, types_, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        d = kwargs.get("device")
        if d is not None and str(d).startswith("cuda"):
            kwargs["device"] = "cpu"
        return func(*args, **kwargs)


def make_inputs():
    xi = [[0, 0, 0, 0, 0, 0],
          [0.12, -0.05, 0.04, 0.01, -0.03, 0.02],
          [-0.10, 0.08, -0.06, -0.02, 0.025, -0.015],
          [0.05, 0.03, -0.8, 0.01, 0.01, 0.03],
          [-0.03, 0.02, 0.45, 0.0, -0.01, -0.01]]
    scale = {1: [(8, 26, 10, 30, 0.6)], 2: [(30, 50, 40, 66, 0.7)], 4: [(20, 34, 26, 44, 0.09)]}
    inp = mf.make_case(H, W, C, xi, depth_scale=scale, seed=7, noise=NOISE)
    inp["disps"][0, 40:48, 8:20] = 0.0
    inp["disps"][2, 5:12, 50:60] = 0.0
    inp["mask"] = np.ones((len(xi), H, W), bool)
    inp["mask"][0, 2:6, 60:70] = False  # (already cleared: stays cleared)
    return inp


def load_reference():
    sys.modules["lietorch"] = lr.lietorch_standin()

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    stub("droid_backends")
    src = stub("src")
    src.__path__ = []
    for pkg in ("src.geom", "src.modules", "src.utils", "src.utils.dyn_uncertainty"):
        stub(pkg).__path__ = []
    stub("src.geom.ba")
    stub("src.modules.droid_net", cvx_upsample=None)
    stub("src.utils.common", align_scale_and_shift=None)
    stub("src.utils.Printer", FontColor=None)
    sys.modules["src.utils.dyn_uncertainty"].mapping_utils = stub("src.utils.dyn_uncertainty.mapping_utils")
    for name, rel in (("src.geom.projective_ops", ("src", "geom", "projective_ops.py")),
                      ("src.depth_video", ("src", "depth_video.py"))):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    sys.modules["src.geom"].projective_ops = sys.modules["src.geom.projective_ops"]
    return sys.modules["src.depth_video"].DepthVideo


def run_reference(inp):
    DepthVideo = load_reference()
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(1)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    num = inp["poses"].shape[0]
    video = types.SimpleNamespace(
        cfg={"tracking": {"nb_ref_frame_metric_depth_filtering": 6}}, device="cpu", down_scale=8,
        poses=t(inp["poses"]), mono_disps_up=t(inp["disps"]), disps_up=torch.zeros(num, H, W),
        mono_disps_mask_up=torch.from_numpy(inp["mask"].copy()), intrinsics=t(inp["intrinsics"])[None].repeat(num, 1),
        dino_feats=t(inp["dino"]))
    # the graph's edges: (IDX, j) for every neighbour, among edges of other frames
    ii = torch.tensor([IDX] * len(JJ) + [1, 2], dtype=torch.int64)
    jj = torch.tensor(JJ + [2, 1], dtype=torch.int64)
    with CudaToCpu():
        DepthVideo.filter_high_err_mono_depth(video, IDX, ii, jj)
    return video.mono_disps_mask_up.numpy()


def main():
    inp = make_inputs()
    ref = mf.filter_mono_depth(inp["poses"], inp["disps"], inp["mask"], inp["intrinsics"], inp["dino"], IDX, JJ)
    acc, ina, amb = ref["accurate"], ref["inaccurate"], ref["ambiguous"]
    share = ref["matched"] / ref["valid"]
    print(f"valid {ref['valid']} of {ref['candidates']}, matched share {share:.3f}, collisions {ref['collisions']}, "
          f"valid with Z < 0.1: {ref['low_z_valid']}")
    print(f"cleared {int((inp['mask'][IDX] & ~ref['mask']).sum())} pixels, ambiguous {int(amb.sum())} of {H * W} "
          f"({amb.mean():.3%})")
    for a, name in ((acc == 0, "0"), (acc == 1, "1"), (acc >= 2, ">=2")):
        for b, nb in ((ina == 0, "0"), (ina >= 1, ">=1")):
            n = int((a & b).sum())
            print(f"  accurate {name}, inaccurate {nb}: {n}")
            assert n > 0, "every combination of the counts has to occur"
    assert 0.2 < share < 0.95
    assert ref["collisions"] >= 100
    assert ref["low_z_valid"] >= 1
    assert amb.mean() <= mf.AMBIGUITY_CAP

    masks = run_reference(inp)
    assert np.array_equal(masks[1:], inp["mask"][1:]), "only row idx may change"
    assert np.array_equal(masks[IDX], ref["mask"]), int((masks[IDX] != ref["mask"]).sum())
    print("the reference's mask equals the restatement's")
    path = os.path.join(HERE, "ref_mono_filter.npz")
    np.savez_compressed(path, poses=inp["poses"], disps=inp["disps"], mask=inp["mask"], intrinsics=inp["intrinsics"],
                        dino=inp["dino"], idx=np.int64(IDX), jj=np.asarray(JJ, np.int64), mask_out=masks[IDX])
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
