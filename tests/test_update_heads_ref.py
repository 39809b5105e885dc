"""CPU tests of the oracle of the update operator's output heads
(tests/_update_heads_ref.py) against the recorded outputs of the reference's own
modules (tests/golden/ref_update_heads.npz, made by
tests/golden/make_update_heads_fixtures.py), and of the packed weight layout
(wgsr.frontend.pack_conv3x3 / unpack_conv3x3).
"""
import os

import numpy as np
import pytest
import torch

import _update_heads_ref as hr
from _util import GOLDEN

CASES = ("a", "b")
fixture_case = hr.fixture_case


def test_fixture_holds_arrays_only():
    z = np.load(os.path.join(GOLDEN, "ref_update_heads.npz"), allow_pickle=False)
    for k in z.files:
        assert z[k].dtype in (np.float16, np.float32, np.float64, np.int64), (k, z[k].dtype)
    assert list(z["a_ii"]) == [2, 0, 2, 5, 0] and list(z["b_ii"]) == [1, 1, 1, 3]
    assert z["a_net"].shape == (5, 32, 3, 5) and z["b_net"].shape == (4, 32, 9, 11)


@pytest.mark.parametrize("tag", CASES)
def test_plain_float64_oracle_is_the_recorded_reference(tag):
    c = fixture_case(tag)
    h = hr.heads(c["net"], c["P"], round16=False)
    g = hr.graph_agg(c["net"], c["ix"], c["G"], c["P"], round16=False)
    for name, got in (("delta", h["delta"]), ("weight", h["weight"]), ("eta", g["eta"]), ("feat", g["feat"])):
        rec = c["z"][f"{tag}_{name}"]
        assert got.shape == rec.shape, name
        assert np.abs(got - rec).max() <= 1e-12 * max(1.0, np.abs(rec).max()), name


@pytest.mark.parametrize("tag", CASES)
def test_rounded_oracle_meets_the_recorded_reference_within_r(tag):
    """float16 rounding points in: the outputs move by at most r, the half ulps pushed through the later layers"""
    c = fixture_case(tag)
    h = hr.heads(c["net"], c["P"])
    g = hr.graph_agg(c["net"], c["ix"], c["G"], c["P"])
    assert np.array_equal(hr.round_fp16(h["hidden"]), h["hidden"]) and np.array_equal(hr.round_fp16(g["feat"]), g["feat"])
    worst = {}
    for name, o in (("delta", h), ("weight", h), ("eta", g), ("feat", g)):
        rec = c["z"][f"{tag}_{name}"]
        err, r = np.abs(o[name] - rec), o["r_" + name]
        assert (r > 0).all() and err.max() > 0, name      # the rounding is visible and bounded
        worst[name] = float((err / r).max())
    print(f"\nfixture {tag}: worst |rounded oracle - recorded| / r: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", [(5, 3, 5), (4, 9, 11)], ids=lambda s: "x".join(map(str, s)))
def test_fp32_evaluation_stays_inside_d(shape):
    """The same formulas in fp32 numpy with the same rounding points stay inside d:
    the bound is not too tight to be met honestly.  (An fp32 value that rounds to
    the other float16 neighbour is what the one ulp16 in d is for.)"""
    n, ht, wd = shape
    rng = np.random.default_rng(n * 100 + wd)
    P = hr.make_params(rng)
    net = rng.standard_normal((n, 128, ht, wd)).astype(np.float16)
    ix = np.array([2, 0, 2, 1, 0][:n]) if n == 5 else np.array([0, 0, 0, 1])
    G = int(ix.max()) + 1
    h64, h32 = hr.heads(net, P), hr.heads(net, P, dtype=np.float32)
    g64, g32 = hr.graph_agg(net, ix, G, P), hr.graph_agg(net, ix, G, P, dtype=np.float32)
    worst = {}
    for name, a, b in (("hidden", h64, h32), ("delta", h64, h32), ("weight", h64, h32),
                       ("mean", g64, g32), ("feat", g64, g32), ("eta", g64, g32)):
        d = a["d_" + name]
        assert (d > 0).all(), name
        worst[name] = float((np.abs(a[name] - b[name]) / d).max())
    print(f"\nfp32 evaluation {shape}: worst error / d: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    assert 0.3 < (h64["hidden"] > 0).mean() < 0.7     # about half the ReLUs are active
    print(f"largest d: hidden {h64['d_hidden'].max():.3g}, delta {h64['d_delta'].max():.3g}, "
          f"feat {g64['d_feat'].max():.3g}, eta {g64['d_eta'].max():.3g}")


@pytest.mark.parametrize("c_out", [1, 2, 128, 256])
def test_packed_layout_round_trips(c_out):
    from wgsr import frontend
    g = torch.Generator().manual_seed(c_out)
    w = torch.randn(c_out, 128, 3, 3, generator=g).half()
    b = torch.randn(c_out, generator=g)
    pw, pb = frontend.pack_conv3x3(w, b)
    rows = (c_out + 15) // 16 * 16
    assert pw.dtype == torch.float16 and pw.shape == (rows * 1152,) and pb.dtype == torch.float32 and pb.shape == (rows,)
    w2, b2 = frontend.unpack_conv3x3(pw, pb, c_out)
    assert torch.equal(w2, w) and torch.equal(b2, b)
    # padding rows are zero, in the weights and in the bias
    wall, ball = frontend.unpack_conv3x3(pw, pb, rows)
    assert torch.equal(wall[:c_out], w) and not wall[c_out:].any() and not ball[c_out:].any()
    # the documented index: fragment (rb, tap, ks), lane, j
    for rb, tap, ks, lane, j in ((0, 0, 0, 0, 0), (0, 5, 3, 37, 6), (rows // 16 - 1, 8, 2, 63, 7)):
        row, ci = 16 * rb + (lane & 15), 32 * ks + 8 * (lane >> 4) + j
        want = w[row, ci, tap // 3, tap % 3] if row < c_out else torch.tensor(0.0).half()
        assert pw[(((rb * 9 + tap) * 4 + ks) * 64 + lane) * 8 + j] == want
    # a float32 parameter holding the same values packs to the same pair, and the pair is kept
    pw32, pb32 = frontend.pack_conv3x3(w.float(), b)
    assert torch.equal(pw32, pw) and torch.equal(pb32, pb)
    assert frontend.pack_conv3x3(w, b)[0] is pw


def test_update_heads_holder_from_state_dict():
    from wgsr import frontend
    rng = np.random.default_rng(3)
    P = hr.make_params(rng)
    sd = {}
    for name, (w, b) in P.items():
        sd[f"update.{name}.weight"], sd[f"update.{name}.bias"] = torch.from_numpy(w), torch.from_numpy(b)
    p = frontend.UpdateHeads.from_state_dict(sd)
    hw, hb = frontend.unpack_conv3x3(*p.hidden, 256)
    assert torch.equal(hw[:128], sd["update.delta.0.weight"]) and torch.equal(hw[128:], sd["update.weight.0.weight"])
    assert torch.equal(hb[128:], sd["update.weight.0.bias"])
    assert p.delta[1].numel() == 16 and p.eta[1].numel() == 16 and p.conv2[1].numel() == 128
    assert torch.equal(frontend.unpack_conv3x3(*p.eta, 1)[0], sd["update.agg.eta.0.weight"])
    with pytest.raises(ValueError, match="convolution"):
        frontend.pack_conv3x3(torch.zeros(128, 64, 3, 3), torch.zeros(128))
