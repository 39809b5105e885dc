"""CPU tests of the DINO-consistency filter of the metric depth prior.

* The float64 restatement (tests/_mono_filter_ref.py) reproduces the mask that
  the reference's own ``DepthVideo.filter_high_err_mono_depth`` gave on the
  inputs of tests/golden/ref_mono_filter.npz
  (tests/golden/make_mono_filter_fixtures.py), exactly.
* The fixture exercises what it was built for, and its ambiguous targets stay
  under the cap the GPU test relies on.
* ``wgsr.frontend.filter_mono_depth`` raises for host tensors, wrong dtypes and
  wrong shapes before any launch (no GPU is needed to see that).
"""
import os

import numpy as np
import pytest
import torch

import _mono_filter_ref as mf
from _util import GOLDEN

_cache = {}


def fixture():
    if not _cache:
        z = np.load(os.path.join(GOLDEN, "ref_mono_filter.npz"))
        inp = {k: z[k] for k in ("poses", "disps", "mask", "intrinsics", "dino")}
        inp["idx"], inp["jj"] = int(z["idx"]), z["jj"]
        _cache["inp"], _cache["mask_out"] = inp, z["mask_out"]
        _cache["ref"] = mf.filter_mono_depth(**inp)
    return _cache["inp"], _cache["ref"], _cache["mask_out"]


def test_restatement_matches_the_reference_mask():
    inp, ref, mask_out = fixture()
    for k in ("poses", "disps", "intrinsics", "dino"):
        assert inp[k].dtype == np.float32, k
    assert mask_out.dtype == bool and mask_out.shape == inp["disps"].shape[1:]
    np.testing.assert_array_equal(ref["mask"], mask_out)
    # the filter only ever clears, and it cleared something
    assert not (mask_out & ~inp["mask"][inp["idx"]]).any()
    assert (inp["mask"][inp["idx"]] & ~mask_out).sum() >= 100


def test_fixture_covers_its_cases():
    inp, ref, _ = fixture()
    H, W = inp["disps"].shape[1:]
    assert (H, W) == (58, 75) and inp["dino"].shape[1:] == (4, 5, 384)
    acc, ina = ref["accurate"], ref["inaccurate"]
    for a in (acc == 0, acc == 1, acc >= 2):
        for b in (ina == 0, ina >= 1):
            assert (a & b).any()
    assert ref["collisions"] >= 100
    assert ref["low_z_valid"] >= 1
    assert 0.2 < ref["matched"] / ref["valid"] < 0.95
    assert (inp["disps"][inp["idx"]] == 0).any()
    assert ref["ambiguous"].mean() <= mf.AMBIGUITY_CAP


def test_upsample_is_torch_bilinear():
    """the restatement's sampling is F.interpolate(mode='bilinear', align_corners=False)"""
    rng = np.random.default_rng(0)
    for (hd, wd, H, W) in ((4, 5, 58, 75), (2, 3, 28, 42), (1, 1, 14, 15)):
        f = rng.standard_normal((hd, wd, 3))
        want = torch.nn.functional.interpolate(torch.from_numpy(f).permute(2, 0, 1)[None], (H, W), mode="bilinear")
        np.testing.assert_allclose(mf.upsample(f, H, W), want[0].permute(1, 2, 0).numpy(), rtol=0, atol=1e-13)


def _args(N=3, H=28, W=42, C=16):
    return dict(poses=torch.zeros(N, 7), mono_disps_up=torch.ones(N, H, W),
                mono_mask_up=torch.ones(N, H, W, dtype=torch.bool), intrinsics=torch.tensor([4.0, 4.0, 2.6, 1.7]),
                dino_feats=torch.zeros(N, H // 14, W // 14, C), idx=0, jj=torch.tensor([1, 2]))


def test_argument_checks_raise_before_any_launch():
    from wgsr.frontend import filter_mono_depth

    # host tensors: a host pointer must never reach a kernel
    a = _args()
    with pytest.raises(RuntimeError, match="poses: expected a HIP device tensor"):
        filter_mono_depth(**a)
    assert a["mono_mask_up"].all()

    def bad(exc, match, **change):
        b = _args()
        b.update(change)
        with pytest.raises(exc, match=match):
            filter_mono_depth(**b)

    bad(RuntimeError, r"poses must be a float32 tensor of dimensions \(N, 7\)", poses=torch.zeros(3, 6))
    bad(RuntimeError, r"poses must be a float32", poses=torch.zeros(3, 7, dtype=torch.float64))
    bad(RuntimeError, r"mono_disps_up must be a float32", mono_disps_up=torch.ones(3, 28, 42, dtype=torch.float16))
    bad(RuntimeError, r"mono_disps_up must be a float32 tensor of dimensions \(N, H, W\)",
        mono_disps_up=torch.ones(28, 42))
    bad(RuntimeError, r"mono_mask_up must be a bool tensor", mono_mask_up=torch.ones(3, 28, 42))
    bad(RuntimeError, r"mono_mask_up must be a bool tensor", mono_mask_up=torch.ones(3, 28, 41, dtype=torch.bool))
    bad(RuntimeError, r"dino_feats must be a float32", dino_feats=torch.zeros(3, 2, 3, 16, dtype=torch.float16))
    bad(ValueError, r"dino_feats must be \(N, 2, 3, C\)", dino_feats=torch.zeros(3, 3, 3, 16))   # hd != H // 14
    bad(ValueError, r"dino_feats must be \(N, 2, 3, C\)", dino_feats=torch.zeros(3, 2, 2, 16))   # wd != W // 14
    bad(ValueError, r"multiple of 4", dino_feats=torch.zeros(3, 2, 3, 6))
    bad(RuntimeError, r"intrinsics must have 4 elements", intrinsics=torch.ones(3))
    bad(RuntimeError, r"jj must be a 1-D", jj=torch.tensor([[1, 2]]))
    bad(RuntimeError, r"jj must be a 1-D", jj=torch.tensor([1.0]))
    bad(RuntimeError, r"idx = 3 must index frames \[0, 3\)", idx=3)
    bad(RuntimeError, r"idx = -1 must index", idx=-1)
    with torch.enable_grad():
        bad(NotImplementedError, "inference only", mono_disps_up=torch.ones(3, 28, 42, requires_grad=True))
