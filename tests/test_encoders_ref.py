"""CPU tests of the oracle of the update operator's two encoders
(tests/_encoders_ref.py) against the recorded outputs of the reference's own
modules (tests/golden/ref_encoders.npz, made by
tests/golden/make_encoders_fixtures.py), of the packed first-layer layouts
(wgsr.frontend.pack_conv1x1_196 / pack_conv7x7_4, UpdateEncoders), and of the
chain of the three oracles against the recorded ``UpdateModule.forward``
(tests/golden/ref_update_operator.npz, make_update_operator_fixtures.py).
"""
import os

import numpy as np
import pytest
import torch

import _encoders_ref as er
from _util import GOLDEN

CASES = ("a", "b")
ENCODERS = ("corr", "flow")
_oracle = {}


def _oracles(tag):
    """{encoder: (plain float64, rounded)} of a fixture case, computed once"""
    if tag not in _oracle:
        c = er.fixture_case(tag)
        _oracle[tag] = {k: (f(c[k], c["P"], round16=False), f(c[k], c["P"]))
                        for k, f in (("corr", er.corr_encoder), ("flow", er.flow_encoder))}
    return _oracle[tag]


def _rows(name, m):
    return m[:, er.FIXTURE_HIDDEN_ROWS] if name == "hidden" else m


def test_fixtures_hold_arrays_only():
    path = os.path.join(GOLDEN, "ref_encoders.npz")
    assert os.path.getsize(path) <= 400 * 1024
    z = np.load(path, allow_pickle=False)
    for k in z.files:
        assert z[k].dtype == np.float64, (k, z[k].dtype)
    assert z["a_corr_out"].shape == (2, 128, 3, 5) and z["b_flow_out"].shape == (1, 64, 6, 18)
    assert z["a_flow_hidden"].shape == (2, 64, 3, 5) and z["b_corr_hidden"].shape == (1, 64, 6, 18)
    z = np.load(er.OP_FIXTURE, allow_pickle=False)
    assert os.path.getsize(er.OP_FIXTURE) <= 400 * 1024
    assert sorted(z.files) == ["a_delta", "a_eta", "a_feat", "a_net", "a_weight", "b_delta", "b_net", "b_weight"]
    assert all(z[k].dtype == np.float64 for k in z.files)


@pytest.mark.parametrize("tag", CASES)
def test_plain_float64_oracle_is_the_recorded_reference(tag):
    c = er.fixture_case(tag)
    for enc in ENCODERS:
        plain = _oracles(tag)[enc][0]
        for name in ("hidden", "out"):
            got, rec = _rows(name, plain[name]), c["z"][f"{tag}_{enc}_{name}"]
            assert got.shape == rec.shape, (enc, name)
            assert np.abs(got - rec).max() <= 1e-12 * max(1.0, np.abs(rec).max()), (enc, name)


@pytest.mark.parametrize("tag", CASES)
def test_rounded_oracle_meets_the_recorded_reference_within_r(tag):
    """float16 rounding points in: the values move by at most r, the hidden half ulp pushed through the second layer"""
    c = er.fixture_case(tag)
    worst = {}
    for enc in ENCODERS:
        o = _oracles(tag)[enc][1]
        for name in ("hidden", "out"):
            assert np.array_equal(er.round_fp16(o[name]), o[name]), (enc, name)
            rec = c["z"][f"{tag}_{enc}_{name}"]
            err, r = np.abs(_rows(name, o[name]) - rec), _rows(name, o["r_" + name])
            live = rec > 0
            assert (r[live] > 0).all() and err.max() > 0, (enc, name)      # the rounding is visible and bounded
            assert (err <= r).all(), (enc, name)
            worst[f"{enc} {name}"] = float((err[live] / r[live]).max())
    print(f"\nfixture {tag}: worst |rounded oracle - recorded| / r: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 9, 17)], ids=lambda s: "x".join(map(str, s)))
def test_fp32_evaluation_stays_inside_d(shape):
    """The same formulas in fp32 numpy with the same rounding points stay inside d"""
    n, ht, wd = shape
    rng = np.random.default_rng(n * 100 + wd)
    P = er.make_params(rng)
    corr, flow = er.make_inputs(rng, n, ht, wd)
    worst = {}
    for enc, f, x in (("corr", er.corr_encoder, corr), ("flow", er.flow_encoder, flow)):
        a, b = f(x, P), f(x, P, dtype=np.float32)
        for name in ("hidden", "out"):
            d = a["d_" + name]
            assert (d > 0).all(), (enc, name)
            worst[f"{enc} {name}"] = float((np.abs(a[name] - b[name]) / d).max())
    print(f"\nfp32 evaluation {shape}: worst error / d: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", er.GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_about_half_the_outputs_are_positive(shape):
    """At the GPU tests' shapes and inputs a dead ReLU cannot hide an error: between 0.2 and 0.8 of the elements of
    each layer are positive."""
    c = er.shape_case(shape)
    for enc in ENCODERS:
        for name in ("hidden", "out"):
            frac = float((c[enc][name] > 0).mean())
            assert 0.2 <= frac <= 0.8, (enc, name, frac)


def test_first_layer_layouts_round_trip():
    from wgsr import frontend
    g = torch.Generator().manual_seed(196)
    b = torch.randn(128, generator=g)
    w = torch.randn(128, 196, 1, 1, generator=g).half()
    pw, pb = frontend.pack_conv1x1_196(w, b)
    assert pw.dtype == torch.float16 and pw.shape == (8 * 7 * 64 * 8,) and pb.dtype == torch.float32
    w2, b2 = frontend.unpack_conv1x1_196(pw, pb)
    assert torch.equal(w2, w) and torch.equal(b2, b)
    for rb, ks, lane, j in ((0, 0, 0, 0), (3, 5, 37, 6), (7, 6, 0, 3), (7, 6, 0, 4), (7, 6, 63, 7), (2, 6, 16, 0)):
        ch = 32 * ks + 8 * (lane >> 4) + j
        want = w[16 * rb + (lane & 15), ch, 0, 0] if ch < 196 else torch.tensor(0.0).half()
        assert pw[((rb * 7 + ks) * 64 + lane) * 8 + j] == want
    assert pw.view(8, 7, 4, 16, 8)[:, 6, 0, :, 4:].eq(0).all() and pw.view(8, 7, 4, 16, 8)[:, 6, 1:].eq(0).all()
    assert frontend.pack_conv1x1_196(w, b)[0] is pw      # the pair is kept

    w = torch.randn(128, 4, 7, 7, generator=g).half()
    pw, pb = frontend.pack_conv7x7_4(w, b)
    assert pw.dtype == torch.float16 and pw.shape == (8 * 7 * 64 * 8,) and pb.dtype == torch.float32
    w2, b2 = frontend.unpack_conv7x7_4(pw, pb)
    assert torch.equal(w2, w) and torch.equal(b2, b)
    for rb, ks, lane, j in ((0, 0, 0, 0), (3, 5, 37, 6), (7, 6, 63, 3), (7, 6, 63, 4), (1, 2, 48, 7)):
        kx, ci = 2 * (lane >> 4) + (j >> 2), j & 3
        want = w[16 * rb + (lane & 15), ci, ks, kx] if kx < 7 else torch.tensor(0.0).half()
        assert pw[((rb * 7 + ks) * 64 + lane) * 8 + j] == want
    assert pw.view(8, 7, 4, 16, 8)[:, :, 3, :, 4:].eq(0).all()      # kx = 7
    with pytest.raises(ValueError, match="first layer"):
        frontend.pack_conv1x1_196(torch.zeros(128, 200, 1, 1), b)
    with pytest.raises(ValueError, match="first layer"):
        frontend.pack_conv7x7_4(torch.zeros(128, 4, 3, 3), b)
    with pytest.raises(ValueError, match="packed first layer"):
        frontend.unpack_conv7x7_4(pw[:-8], pb)


def test_update_encoders_holder_from_state_dict():
    from wgsr import frontend
    P = er.make_params(np.random.default_rng(5))
    sd = {}
    for name, (w, b) in P.items():
        sd[f"update.{name}.weight"], sd[f"update.{name}.bias"] = torch.from_numpy(w), torch.from_numpy(b)
    p = frontend.UpdateEncoders.from_state_dict(sd)
    assert torch.equal(frontend.unpack_conv1x1_196(*p.corr1)[0], sd["update.corr_encoder.0.weight"])
    assert torch.equal(frontend.unpack_conv7x7_4(*p.flow1)[0], sd["update.flow_encoder.0.weight"])
    assert torch.equal(frontend.unpack_conv3x3(*p.corr2, 128)[0], sd["update.corr_encoder.2.weight"])
    w2, b2 = frontend.unpack_conv3x3(*p.flow2, 64)
    assert torch.equal(w2, sd["update.flow_encoder.2.weight"]) and torch.equal(b2, sd["update.flow_encoder.2.bias"])
    assert p.flow2[1].numel() == 64 and p.corr2[1].numel() == 128
    with pytest.raises(ValueError, match="flow_encoder.2 must be"):
        frontend.UpdateEncoders.from_state_dict({**sd, "update.flow_encoder.2.weight": torch.zeros(128, 128, 3, 3)})


@pytest.mark.parametrize("tag", ("a", "b"))
def test_chained_oracles_are_the_recorded_update_operator(tag):
    """encoders -> ConvGRU -> heads / graph_agg, all plain float64: which encoder feeds which source of the GRU,
    the [..., :2] slice, the factor 0.01 and the ``flow=None`` form"""
    Pe, Pg, Ph, x = er.op_fixture_inputs(tag)
    z = np.load(er.OP_FIXTURE, allow_pickle=False)
    got = er.update_operator(x["net"], x["inp"], x["corr"], x["flow"], x["ii"], Pe, Pg, Ph, round16=False)
    names = ("net", "delta", "weight") + (("eta", "feat") if x["ii"] is not None else ())
    assert (x["flow"] is None) == (tag == "b") and sorted(got) == sorted(names)
    for name in names:
        rec = z[f"{tag}_{name}"]
        assert got[name].shape == rec.shape, name
        assert np.abs(got[name] - rec).max() <= 1e-12 * max(1.0, np.abs(rec).max()), name
    # the wiring is visible: the encoders' outputs swapped into each other's place cannot even be formed (128
    # against 64 channels), and a flow of zeros is not a flow left out of the GRU
    assert np.abs(z[f"{tag}_net"]).max() > 0.5
