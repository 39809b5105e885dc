"""CPU tests of the feature / context encoders' oracle (tests/_basic_encoder_ref.py)
against the recorded outputs of the reference's own BasicEncoder
(tests/golden/ref_basic_encoder.npz), and of the parts of
wgsr.frontend.feature_encoder / context_encoder that need no device: the packed
layouts, the map sizes and the argument errors."""
import numpy as np
import pytest
import torch

import _basic_encoder_ref as br

HOOKED = {"stem": "R0", "layer1": "A5", "layer2": "A9", "layer3": "A13"}


def _pre_activation(c, ev):
    """the head's output before the caller's split, from the oracle's last staged operand"""
    return br.conv2d(ev["A13"], *c["P"]["conv2"])


@pytest.mark.parametrize("tag", ["f", "c"])
def test_plain_oracle_is_the_reference(tag):
    c = br.fixture_case(tag)
    z, pl = c["z"], c["plain"]
    for key, name in HOOKED.items():
        assert np.abs(pl[name][:, br.FIXTURE_EVEN] - z[f"{tag}_{key}"]).max() <= 1e-10, key
    down = br._norm(pl["Rd5"], pl.get("Sd5"))
    assert np.abs(down[:, br.FIXTURE_EVEN] - z[f"{tag}_down2"]).max() <= 1e-10
    if tag == "f":
        assert np.abs(pl["out"] - z["f_out"]).max() <= 1e-10
    else:
        assert np.abs(_pre_activation(c, pl) - z["c_out"]).max() <= 1e-10
        assert np.abs(pl["net"] - np.tanh(z["c_out"][:, :128])).max() <= 1e-10
        assert np.abs(pl["inp"] - np.maximum(z["c_out"][:, 128:], 0)).max() <= 1e-10


@pytest.mark.parametrize("tag", ["f", "c"])
def test_rounded_oracle_is_within_its_r(tag):
    c = br.fixture_case(tag)
    z, ro = c["z"], c["rounded"]
    if tag == "f":
        pairs = [(ro["out"], z["f_out"], ro["r_out"])]
    else:
        pairs = [(ro["net"], np.tanh(z["c_out"][:, :128]), ro["r_net"]),
                 (ro["inp"], np.maximum(z["c_out"][:, 128:], 0), ro["r_inp"])]
    for got, ref, r in pairs:
        assert np.isfinite(r).all() and (np.abs(got - ref) <= r).all()
        assert got.astype(np.float16).astype(np.float64).tolist() == got.tolist()      # float16 values
    # and the rounding points are there: the two evaluations differ, by a few ulp16 of the output's size
    e16 = np.sqrt(np.mean((pairs[0][0] - c["plain"]["out" if tag == "f" else "net"]) ** 2))
    assert 0 < e16 < 0.05


def test_cnet_head_stays_off_saturation():
    """the scaled head's pre-activation rms lies in [0.5, 2] (at the fixture's case and at the smallest and an odd GPU
    shape), and so tanh is not saturated"""
    cases = [br.fixture_case("c")] + [br.shape_case("none", s) for s in br.GPU_SHAPES[:2]]
    for c in cases:
        pre = _pre_activation(c, c["plain"])
        rms = np.sqrt((pre ** 2).mean())
        assert 0.5 <= rms <= 2.0, rms
        assert (np.abs(c["plain"]["net"]) < 0.999).mean() > 0.9


def test_instance_norm_variances_are_far_above_eps():
    c = br.shape_case("instance", br.GPU_SHAPES[0])
    least = min((1.0 / v[1] ** 2 - br.EPS).min() for k, v in c["plain"].items() if k.startswith("S"))
    assert least > 100 * br.EPS, least


@pytest.mark.parametrize("shape", [(16, 24), (37, 53), (21, 27), (1, 1), (8, 9)])
def test_output_sizes_are_ceil(shape):
    from wgsr import frontend
    H, W = shape
    want = tuple((-(-H // s), -(-W // s)) for s in (2, 4, 8))
    assert frontend.be_sizes(H, W) == want == tuple(br.sizes(H, W))
    x = np.zeros((1, 3, H, W))
    assert br.conv2d(x, np.zeros((2, 3, 7, 7)), None, 2).shape[2:] == want[0]
    y = np.zeros((1, 4) + want[0])
    assert br.conv2d(y, np.zeros((2, 4, 3, 3)), None, 2).shape[2:] == want[1]
    assert br.conv2d(y, np.zeros((2, 4, 1, 1)), None, 2).shape[2:] == want[1]


def test_stride_two_reads_the_centre_tap_of_the_three_by_three():
    """the 1 x 1 stride-2 convolution equals the 3 x 3 stride-2 one whose only tap is the centre, at odd sizes too"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 4, 5, 7))
    w1 = rng.standard_normal((3, 4, 1, 1))
    w3 = np.zeros((3, 4, 3, 3))
    w3[:, :, 1, 1] = w1[:, :, 0, 0]
    one = br.conv2d(x, w1, None, 2)      # (the sums run in another order: equal up to float64 rounding)
    assert one.shape == (2, 3, 3, 4) and np.abs(one - br.conv2d(x, w3, None, 2)).max() <= 1e-12
    assert np.abs(one - np.einsum("oc,nchw->nohw", w1[:, :, 0, 0], x[:, :, ::2, ::2])).max() <= 1e-12


def test_pack_round_trips():
    from wgsr import frontend
    rng = np.random.default_rng(3)
    w = torch.from_numpy(rng.standard_normal((32, 3, 7, 7)).astype(np.float16))
    b = torch.from_numpy(rng.standard_normal(32).astype(np.float32))
    pw, pb = frontend.pack_stem7x7(w, b)
    assert pw.dtype == torch.float16 and pw.numel() == 2 * 5 * 64 * 8 and pb.dtype == torch.float32
    w2, b2 = frontend.unpack_stem7x7(pw, pb)
    assert torch.equal(w2, w) and torch.equal(b2, b)
    # the documented element: ((rb 5 + ks) 64 + lane) 8 + j <-> product k = 32 ks + 8 (lane >> 4) + j = 21 ky + 3 kx + ci
    flat = pw.view(2, 5, 64, 8)
    for rb, ks, lane, j in ((0, 0, 0, 0), (1, 2, 37, 5), (1, 4, 15, 2), (0, 4, 63, 7)):
        k = 32 * ks + 8 * (lane >> 4) + j
        want = w[16 * rb + (lane & 15), k % 3, k // 21, k % 21 // 3] if k < 147 else 0.0
        assert float(flat[rb, ks, lane, j]) == float(want), (rb, ks, lane, j)
    assert not flat.view(2, 5, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(32, 160)[:, 147:].any()
    for c_out, c_in in ((128, 128), (256, 128), (64, 32)):
        w = torch.from_numpy(rng.standard_normal((c_out, c_in, 1, 1)).astype(np.float16))
        b = torch.from_numpy(rng.standard_normal(c_out).astype(np.float32))
        pw, pb = frontend.pack_conv1x1(w, b)
        assert pw.numel() == c_out * c_in
        w2, b2 = frontend.unpack_conv1x1(pw, pb, c_in)
        assert torch.equal(w2, w) and torch.equal(b2, b)
        flat = pw.view(c_out // 16, c_in // 32, 64, 8)
        assert float(flat[1, c_in // 32 - 1, 21, 3]) == float(w[16 + 5, c_in - 32 + 8 + 3, 0, 0])
    with pytest.raises(ValueError, match="stem must be"):
        frontend.pack_stem7x7(torch.zeros(32, 4, 7, 7), torch.zeros(32))
    with pytest.raises(ValueError, match="1 x 1 convolution must be"):
        frontend.pack_conv1x1(torch.zeros(64, 48, 1, 1), torch.zeros(64))
    with pytest.raises(ValueError, match="not a packed"):
        frontend.unpack_conv1x1(pw, pb, 96)


def _state_dict(P, prefix=""):
    sd = {}
    for name, (w, b) in P.items():
        sd[f"{prefix}{name}.weight"] = torch.from_numpy(np.ascontiguousarray(w))
        sd[f"{prefix}{name}.bias"] = torch.from_numpy(np.ascontiguousarray(b))
    return sd


def test_parameters_pack_once_from_every_prefix():
    from wgsr import frontend
    for norm, prefix in (("instance", "fnet."), ("none", "cnet."), ("instance", "")):
        _, P, _ = br.fixture_inputs("f" if norm == "instance" else "c")
        sd = _state_dict(P, prefix)
        p = frontend.BasicEncoder.from_state_dict(sd, prefix=prefix, norm=norm)
        assert p.norm == norm and p.out_dim == br.OUT[norm] and p.head[1].numel() == br.OUT[norm]
        assert sorted(p.convs) == sorted(f"{b}.{k}" for b in br.BLOCKS for k in ("conv1", "conv2"))
        w3, w1, bias, rows3, rows1 = p.convs["layer2.0.conv1"]
        assert (rows3, rows1) == (64, 64) and bias.numel() == 128 and w1.numel() == 64 * 32
        assert torch.equal(bias[64:], sd[f"{prefix}layer2.0.downsample.0.bias"])
        assert p.convs["layer1.0.conv1"][1] is None and p.convs["layer1.0.conv1"][3:] == (32, 0)
        again = frontend.BasicEncoder.from_state_dict(sd, prefix=prefix, norm=norm)
        assert again.stem[0] is p.stem[0] and again.convs["layer3.1.conv2"][0] is p.convs["layer3.1.conv2"][0]
        got = frontend.unpack_conv3x3_wide(w3, bias[:64], 64, 32)[0]
        assert torch.equal(got, sd[f"{prefix}layer2.0.conv1.weight"])


def test_errors_that_need_no_device():
    from wgsr import frontend
    _, P, images = br.fixture_inputs("f")
    sd = _state_dict(P, "fnet.")
    x = torch.from_numpy(images)
    with pytest.raises(ValueError, match="norm must be"):
        frontend.BasicEncoder.from_state_dict(sd, norm="batch")
    with pytest.raises(ValueError, match="conv2 must be"):
        frontend.BasicEncoder.from_state_dict(sd, prefix="fnet.", norm="none")
    for f in (frontend.feature_encoder, frontend.context_encoder):
        with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
            f(x, sd)
        with torch.enable_grad():
            with pytest.raises(NotImplementedError, match="images requires grad"):
                f(x.clone().requires_grad_(), sd)
    with pytest.raises(ValueError, match="one pixel"):
        frontend.BasicEncoderWorkspace(1, 8, 8, "instance", "cpu")
    with pytest.raises(ValueError, match="norm must be"):
        frontend.BasicEncoderWorkspace(1, 16, 16, "group", "cpu")
