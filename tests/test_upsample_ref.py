"""CPU tests of the float64 oracle of the convex upsampling and its mask head
(tests/_upsample_ref.py) against tests/golden/ref_upsample.npz, the recorded
outputs of the reference's own ``cvx_upsample``, ``upsample_disp`` and
``GraphAgg().upmask`` (tests/golden/make_upsample_fixtures.py).

The oracle must reproduce every recorded float64 output to 1e-12 x max(1,
|ref|): that pins the formula the GPU tests check the kernels against --
neighbour order, zero padding, the sub-position layout of the 576 channels --
and, through the head's logits, the channel order of the reference's module.
"""
import os

import numpy as np
import pytest

import _upsample_ref as ur
from _util import GOLDEN

CASES = {"a": (2, 3, 5), "b": (1, 9, 11)}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "ref_upsample.npz"))


def _close(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert ref.dtype == np.float64
    return np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("tag", sorted(CASES))
def test_fixture_inputs_are_what_the_gpu_tests_feed(fx, tag):
    n, ht, wd = CASES[tag]
    assert fx[f"{tag}_mask"].dtype == np.float16 and fx[f"{tag}_mask"].shape == (n, 576, ht, wd)
    assert fx[f"{tag}_data"].dtype == np.float32 and fx[f"{tag}_data"].shape == (n, ht, wd, 2)
    assert np.isfinite(fx[f"{tag}_mask"]).all()
    assert fx[f"{tag}_data"].min() >= 0.1 and fx[f"{tag}_data"].max() <= 1.1


@pytest.mark.parametrize("tag", sorted(CASES))
def test_oracle_reproduces_cvx_upsample(fx, tag):
    data, mask = fx[f"{tag}_data"], fx[f"{tag}_mask"]
    assert _close(ur.cvx_upsample(data[..., :1], mask)["up"], fx[f"{tag}_up1"])
    assert _close(ur.cvx_upsample(data, mask)["up"], fx[f"{tag}_up2"])
    # upsample_disp: [1, n, ht, wd] -> [1, n, 8 ht, 8 wd]
    assert _close(ur.cvx_upsample(data[..., :1], mask)["up"][None, ..., 0], fx[f"{tag}_disp_up"])


@pytest.mark.parametrize("tag", sorted(CASES))
def test_channels_agree_and_weights_are_convex(fx, tag):
    data, mask = fx[f"{tag}_data"], fx[f"{tag}_mask"]
    r1, r2 = ur.cvx_upsample(data[..., :1], mask), ur.cvx_upsample(data, mask)
    np.testing.assert_array_equal(r1["up"][..., 0], r2["up"][..., 0])
    # positive data: the magnitude is the value itself; a convex combination stays within the neighbours' range
    np.testing.assert_allclose(r2["mag"], r2["up"], rtol=1e-14)
    assert (r2["spread"] >= 0).all() and (r2["up"] <= data.max() + 1e-12).all() and (r2["up"] >= 0).all()
    # at a border the padding zeros belong to the neighbourhood: the spread there is the largest neighbour
    assert r1["spread"][0, 0, 0, 0] == ur.neighbours(data[..., :1].astype(np.float64))[0, :, 0, 0, 0].max()


@pytest.mark.parametrize("tag", sorted(CASES))
def test_update_path_differs_by_its_fp16_weights(fx, tag):
    """The recorded ``FactorGraph.update`` variant rounds the softmax weights
    to float16: it lies within 2^-11 mag + 9 x 2^-12 max|d| (the rounded
    weights need not sum to 1) + fp32 summation error of the oracle."""
    data, mask = fx[f"{tag}_data"], fx[f"{tag}_mask"]
    r = ur.cvx_upsample(data[..., :1], mask)
    rec = fx[f"{tag}_up1_update"]
    assert rec.dtype == np.float32
    err = np.abs(rec.astype(np.float64) - r["up"])
    bound = (2.0 ** -11 + 2.0 ** -20) * r["mag"] + 9 * 2.0 ** -12 * np.abs(data).max()
    assert (err <= bound).all(), float((err / bound).max())
    assert err.max() > 2.0 ** -16  # and it is the rounded-weights variant, not the float64 one


def test_oracle_reproduces_the_head(fx):
    h = ur.head(fx["head_feat"], fx["head_weight"], fx["head_bias"])
    assert fx["head_weight"].dtype == np.float16 and fx["head_weight"].shape == (576, 32)
    assert fx["head_bias"].dtype == np.float32 and fx["head_feat"].dtype == np.float16
    assert _close(h["exact"], fx["head_logits"])
    assert _close(ur.cvx_upsample(fx["a_data"][..., :1], h["logits"])["up"], fx["head_up"])
    # the rounding is float16's, and the derived logit bound covers it
    assert np.abs(h["logits"] - h["exact"]).max() <= 0.5 * ur.ulp_fp16(h["exact"]).max()
    assert (np.abs(h["logits"] - h["exact"]) <= ur.logit_delta(h, 32)).all()


def test_ulp_and_perturbation_bound():
    assert ur.ulp_fp16(1.0) == 2.0 ** -10 and ur.ulp_fp16(1.999) == 2.0 ** -10 and ur.ulp_fp16(2.0) == 2.0 ** -9
    assert ur.ulp_fp16(0.0) == 2.0 ** -24 and ur.ulp_fp16(-3.0) == 2.0 ** -9
    # the bound holds for logits moved by up to 2 delta (two sets each within delta of the exact ones)
    rng = np.random.default_rng(3)
    n, ht, wd = 1, 4, 5
    data = rng.uniform(0.1, 1.1, (n, ht, wd, 1))
    mask = 3 * rng.standard_normal((n, 576, ht, wd))
    delta = np.full(mask.shape, 0.01)
    base = ur.cvx_upsample(data, mask)
    bound = ur.perturbation_bound(delta, base["spread"])
    for _ in range(4):
        moved = ur.cvx_upsample(data, mask + 0.02 * rng.choice([-1.0, 1.0], mask.shape))["up"]
        assert (np.abs(moved - base["up"]) <= bound).all()
