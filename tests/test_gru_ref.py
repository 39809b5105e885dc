"""CPU tests of the oracle of the update operator's ConvGRU (tests/_gru_ref.py)
against the recorded outputs of the reference's own module
(tests/golden/ref_gru.npz, made by tests/golden/make_gru_fixtures.py), and of
the wide packed weight layout (wgsr.frontend.pack_conv3x3_wide /
unpack_conv3x3_wide, UpdateGRU).
"""
import os

import numpy as np
import pytest
import torch

import _gru_ref as gr
from _util import GOLDEN

CASES = ("a", "b")
OUTPUTS = ("gbias", "z", "rnet", "out")
_oracle = {}


def _recorded(c, tag, name):
    return c["z"][f"{tag}_" + ("net_out" if name == "out" else name)]


def _rows(name, m):
    return m[:, gr.FIXTURE_ZR_ROWS] if name in ("z", "rnet") else m


def _oracles(tag):
    """(plain float64, rounded) evaluations of a fixture case, computed once"""
    if tag not in _oracle:
        c = gr.fixture_case(tag)
        args = (c["net"], c["inp"], c["corr"], c["flow"], c["P"])
        _oracle[tag] = (gr.gru(*args, round16=False), gr.gru(*args))
    return _oracle[tag]


def test_fixture_holds_arrays_only():
    path = os.path.join(GOLDEN, "ref_gru.npz")
    assert os.path.getsize(path) <= 400 * 1024
    z = np.load(path, allow_pickle=False)
    for k in z.files:
        assert z[k].dtype == np.float64, (k, z[k].dtype)
    assert z["a_net_out"].shape == (2, 128, 3, 5) and z["b_net_out"].shape == (1, 128, 6, 18)
    assert z["a_z"].shape == (2, 64, 3, 5) and z["b_rnet"].shape == (1, 64, 6, 18) and z["b_gbias"].shape == (1, 384)


@pytest.mark.parametrize("tag", CASES)
def test_plain_float64_oracle_is_the_recorded_reference(tag):
    c = gr.fixture_case(tag)
    plain = _oracles(tag)[0]
    for name in OUTPUTS:
        got, rec = _rows(name, plain[name]), _recorded(c, tag, name)
        assert got.shape == rec.shape, name
        assert np.abs(got - rec).max() <= 1e-12 * max(1.0, np.abs(rec).max()), name


@pytest.mark.parametrize("tag", CASES)
def test_rounded_oracle_meets_the_recorded_reference_within_r(tag):
    """float16 rounding points in: the outputs move by at most r, the half ulps pushed through the q stage"""
    c = gr.fixture_case(tag)
    o = _oracles(tag)[1]
    for name in ("z", "rnet", "out"):
        assert np.array_equal(gr.round_fp16(o[name]), o[name]), name
    assert not o["r_gbias"].any()
    worst = {}
    for name in ("z", "rnet", "out"):
        rec = _recorded(c, tag, name)
        err, r = np.abs(_rows(name, o[name]) - rec), _rows(name, o["r_" + name])
        assert (r > 0).all() and err.max() > 0, name      # the rounding is visible and bounded
        worst[name] = float((err / r).max())
    print(f"\nfixture {tag}: worst |rounded oracle - recorded| / r: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 9, 17)], ids=lambda s: "x".join(map(str, s)))
def test_fp32_evaluation_stays_inside_d(shape):
    """The same formulas in fp32 numpy (the kernel's expressions of sigmoid and tanh) with the same rounding
    points stay inside d, end to end and per stage on exactly known inputs."""
    n, ht, wd = shape
    rng = np.random.default_rng(n * 100 + wd)
    P = gr.make_params(rng)
    net, inp, corr, flow = gr.make_inputs(rng, n, ht, wd)
    a, b = gr.gru(net, inp, corr, flow, P), gr.gru(net, inp, corr, flow, P, dtype=np.float32)
    worst = {}
    for name in OUTPUTS:
        d = a["d_" + name]
        assert (d > 0).all(), name
        worst[name] = float((np.abs(a[name] - b[name]) / d).max())
    # per stage, fed the fp32 evaluation's own intermediates as exactly known values
    zr = gr.stage_zr(net, inp, corr, flow, b["gbias"], P)
    q = gr.stage_q(b["rnet"], inp, corr, flow, b["gbias"], b["z"], net, P)
    for name, o in (("z", zr), ("rnet", zr), ("out", q)):
        worst["stage " + name] = float((np.abs(o[name] - b[name]) / o["d_" + name]).max())
        assert (o["d_" + name] <= a["d_" + name]).all(), name     # the stage bounds are the tighter ones
    print(f"\nfp32 evaluation {shape}: worst error / d: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    assert 0.2 < a["z"].mean() < 0.8 and np.abs(a["out"]).max() > 1.0
    print("largest d: " + ", ".join(f"{k} {a['d_' + k].max():.3g}" for k in OUTPUTS))


def test_activation_bounds_cover_the_kernels_expressions():
    """SIG_ABS / TANH_ABS against the float32 expressions over the whole range, saturation included"""
    v = np.concatenate([np.linspace(-100, 100, 200001), np.linspace(-1e-3, 1e-3, 2001)]).astype(np.float32)
    v64 = v.astype(np.float64)
    assert np.abs(gr.sigmoid(v).astype(np.float64) - gr.sigmoid(v64)).max() <= gr.SIG_ABS
    assert np.abs(gr.tanh(v).astype(np.float64) - np.tanh(v64)).max() <= gr.TANH_ABS
    assert gr.tanh(np.float32([60.0, -60.0])).tolist() == [1.0, -1.0]


@pytest.mark.parametrize("c_in", [32, 128, 448])
@pytest.mark.parametrize("c_out", [2, 128, 256])
def test_wide_packed_layout_round_trips(c_out, c_in):
    from wgsr import frontend
    g = torch.Generator().manual_seed(1000 * c_out + c_in)
    w = torch.randn(c_out, c_in, 3, 3, generator=g).half()
    b = torch.randn(c_out, generator=g)
    pw, pb = frontend.pack_conv3x3_wide(w, b)
    rows, KS = (c_out + 15) // 16 * 16, c_in // 32
    assert pw.dtype == torch.float16 and pw.shape == (rows * c_in * 9,) and pb.dtype == torch.float32 and pb.shape == (rows,)
    w2, b2 = frontend.unpack_conv3x3_wide(pw, pb, c_out, c_in)
    assert torch.equal(w2, w) and torch.equal(b2, b)
    wall, ball = frontend.unpack_conv3x3_wide(pw, pb, rows, c_in)
    assert torch.equal(wall[:c_out], w) and not wall[c_out:].any() and not ball[c_out:].any()
    # the documented index: fragment (rb, tap, ks), lane, j
    for rb, tap, ks, lane, j in ((0, 0, 0, 0, 0), (0, 5, KS - 1, 37, 6), (rows // 16 - 1, 8, KS // 2, 63, 7)):
        row, ci = 16 * rb + (lane & 15), 32 * ks + 8 * (lane >> 4) + j
        want = w[row, ci, tap // 3, tap % 3] if row < c_out else torch.tensor(0.0).half()
        assert pw[(((rb * 9 + tap) * KS + ks) * 64 + lane) * 8 + j] == want
    assert frontend.pack_conv3x3_wide(w, b)[0] is pw      # the pair is kept
    if c_in == 128:   # the existing layout is the case KS = 4
        pw4, pb4 = frontend.pack_conv3x3(w, b)
        assert pw4.numpy().tobytes() == pw.numpy().tobytes() and pb4.numpy().tobytes() == pb.numpy().tobytes()


def test_wide_packing_errors():
    from wgsr import frontend
    with pytest.raises(ValueError, match="multiple of 32"):
        frontend.pack_conv3x3_wide(torch.zeros(128, 48, 3, 3), torch.zeros(128))
    with pytest.raises(ValueError, match="convolution"):
        frontend.pack_conv3x3_wide(torch.zeros(128, 64, 1, 1), torch.zeros(128))
    with pytest.raises(ValueError, match="packed pair"):
        frontend.unpack_conv3x3_wide(torch.zeros(16 * 64 * 9).half(), torch.zeros(16), 2, 32)
    # pack_conv3x3 keeps its own check
    with pytest.raises(ValueError, match="convolution"):
        frontend.pack_conv3x3(torch.zeros(128, 64, 3, 3), torch.zeros(128))


def test_update_gru_holder_from_state_dict():
    from wgsr import frontend
    P = gr.make_params(np.random.default_rng(4))
    sd = {}
    for name, (w, b) in P.items():
        sd[f"update.gru.{name}.weight"], sd[f"update.gru.{name}.bias"] = torch.from_numpy(w), torch.from_numpy(b)
    p = frontend.UpdateGRU.from_state_dict(sd)
    zw, zb = frontend.unpack_conv3x3_wide(*p.zr, 256, 448)
    assert torch.equal(zw[:128], sd["update.gru.convz.weight"]) and torch.equal(zw[128:], sd["update.gru.convr.weight"])
    assert torch.equal(zb[:128], sd["update.gru.convz.bias"]) and torch.equal(zb[128:], sd["update.gru.convr.bias"])
    assert torch.equal(frontend.unpack_conv3x3_wide(*p.q, 128, 448)[0], sd["update.gru.convq.weight"])
    # glo_w: w as a one-tap packing (fragment (rb, ks), lane, j), then the three glo matrices as they lie
    assert p.glo_w.dtype == torch.float16 and p.glo_w.shape == (4 * 128 * 128,)
    w = sd["update.gru.w.weight"].view(128, 128)
    for rb, ks, lane, j in ((0, 0, 0, 0), (3, 2, 37, 6), (7, 3, 63, 7)):
        assert p.glo_w[((rb * 4 + ks) * 64 + lane) * 8 + j] == w[16 * rb + (lane & 15), 32 * ks + 8 * (lane >> 4) + j]
    rest = p.glo_w[128 * 128:].view(3, 128, 128)
    for k, name in enumerate(("convz_glo", "convr_glo", "convq_glo")):
        assert torch.equal(rest[k], sd[f"update.gru.{name}.weight"].view(128, 128))
    names = ("w", "convz", "convr", "convq", "convz_glo", "convr_glo", "convq_glo")
    assert torch.equal(p.glo_b, torch.cat([sd[f"update.gru.{k}.bias"] for k in names]))
    with pytest.raises(ValueError, match="convz must be"):
        frontend.UpdateGRU.from_state_dict({**sd, "update.gru.convz.weight": torch.zeros(128, 128, 3, 3)})
