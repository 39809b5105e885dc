"""The float64 oracle of the update operator's two encoders
(UpdateModule.corr_encoder / .flow_encoder, droid_net.py:88-100, 136-137), in
numpy, with a per-output error bound:

    corr [n, 196, ht, wd] -> Conv2d(196, 128, 1) ReLU, Conv2d(128, 128, 3, padding=1) ReLU -> [n, 128, ht, wd]
    flow [n, 4, ht, wd]   -> Conv2d(4, 128, 7, padding=3) ReLU, Conv2d(128, 64, 3, padding=1) ReLU -> [n, 64, ht, wd]

Parameters ``P``: a dict ``name -> (weight, bias)`` with the reference's names
``corr_encoder.0``, ``corr_encoder.2``, ``flow_encoder.0``, ``flow_encoder.2``;
the weights hold float16 values, the biases float32 values.  The inputs hold
float16 values (the kernel rounds a float32 ``flow`` to float16 as it reads it,
autocast's cast: a caller with other values rounds them first).

Rounding points (``round16=True``; they are the kernel's, csrc/droid_encoders.hip,
and autocast's): the hidden layer and the output are rounded to float16 once
each.  ``round16=False`` is the plain float64 evaluation the fixture was
recorded with.  ``dtype=np.float32`` evaluates the same formulas at the
precision of the kernel.

Every value ``v`` comes with two maps of its shape, both derived by first-order
propagation, nothing fitted (the scheme of _update_heads_ref.py):

``d``  the most a kernel that follows the contract can differ from ``v``.  The
       first layer, 196 products accumulated in fp32 and the bias: (196 + 2)
       2^-24 (sum |w| |x| + |b|).  ReLU is 1-Lipschitz.  At the hidden rounding
       point both sides round to float16 and the two roundings may fall on
       either side of a tie: one ulp16, taken at |v| + d.  The hidden d is
       pushed through the second layer as sum |w| d, which adds its own (1152 +
       2) 2^-24 (sum |w| |hidden| + |b|), and the output rounding one more ulp16.
``r``  the most ``v`` (rounding points in) differs from the plain float64
       value: half an ulp16 at each rounding point, pushed through the second
       layer the same way.

So |kernel - oracle| <= d, and |kernel - recorded float64 reference| <= d + r.
A hidden pixel outside the map is zero: the second convolution pads the hidden
layer (it does not evaluate the first layer on a padded input).
"""
from __future__ import annotations

import os

import numpy as np

import _update_heads_ref as hr
from _upsample_ref import round_fp16, ulp_fp16  # noqa: F401  (re-exported)

K1 = 196                     # products per hidden value, in both encoders
U32 = 2.0 ** -24
CORR_PLANES, FLOW_PLANES, HIDDEN = 196, 4, 128
NAMES = ("corr_encoder.0", "corr_encoder.2", "flow_encoder.0", "flow_encoder.2")
SHAPES = {"corr_encoder.0": (128, 196, 1, 1), "corr_encoder.2": (128, 128, 3, 3),
          "flow_encoder.0": (128, 4, 7, 7), "flow_encoder.2": (64, 128, 3, 3)}
FLOW_CLAMP = 64.0            # factor_graph.py clamps motn to [-64, 64]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_encoders.npz")
FIXTURE_CASES = {"a": (2, 3, 5), "b": (1, 6, 18)}
FIXTURE_SEED = {"a": 20251, "b": 20252}
FIXTURE_HIDDEN_ROWS = slice(0, HIDDEN, 2)   # the hidden layers are recorded for the even channels (the file's size)
_fixture = {}


def conv2d(x, w, b=None):
    """x [n, C, ht, wd], w [C_out, C, k, k] (k odd), b [C_out] or None -> [n, C_out, ht, wd]; padding k // 2, in
    x's dtype (each tap one matrix product)"""
    n, C, ht, wd = x.shape
    k = w.shape[2]
    p = k // 2
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    w = w.astype(x.dtype)
    out = np.zeros((n, w.shape[0], ht * wd), x.dtype)
    for ky in range(k):
        for kx in range(k):
            out += np.matmul(w[:, :, ky, kx], xp[:, :, ky:ky + ht, kx:kx + wd].reshape(n, C, ht * wd))
    if b is not None:
        out += b.astype(x.dtype)[None, :, None]
    return out.reshape(n, -1, ht, wd)


def first_layer(x, w, b, round16=True, dtype=np.float64):
    """fp16(ReLU(conv(x) + b)) of an exactly known x -> (hidden, d, r)"""
    x64, w64, b64 = (np.asarray(m, np.float64) for m in (x, w, b))
    v = conv2d(x64.astype(dtype), w64, b64).astype(np.float64)
    d = (K1 + 2) * U32 * (conv2d(np.abs(x64), np.abs(w64)) + np.abs(b64)[None, :, None, None])
    return hr.relu_store16(v, d, np.zeros_like(v), round16)


def encoder(x, first, second, round16=True, dtype=np.float64):
    """Both layers -> dict(hidden, out) with d_* and r_* of each"""
    hid, dh, rh = first_layer(x, *first, round16=round16, dtype=dtype)
    out, do, ro = hr.relu_store16(*hr.conv_layer(hid, *second, dh, rh, dtype), round16)
    return {"hidden": hid, "d_hidden": dh, "r_hidden": rh, "out": out, "d_out": do, "r_out": ro}


def corr_encoder(corr, P, round16=True, dtype=np.float64):
    """corr [n, 196, ht, wd] -> dict(hidden [n, 128, ht, wd], out [n, 128, ht, wd]) and d_* / r_*"""
    return encoder(corr, P["corr_encoder.0"], P["corr_encoder.2"], round16, dtype)


def flow_encoder(flow, P, round16=True, dtype=np.float64):
    """flow [n, 4, ht, wd] -> dict(hidden [n, 128, ht, wd], out [n, 64, ht, wd]) and d_* / r_*"""
    return encoder(flow, P["flow_encoder.0"], P["flow_encoder.2"], round16, dtype)


def make_params(rng):
    """Seeded parameters (``rng``: a Generator or a RandomState) with float16 weight values scaled by 1 / sqrt(K)
    (K = 196 for the first layers, 1152 for the second) and biases 0.1 x normal, so that about half the ReLUs
    are active."""
    P = {}
    for name in NAMES:
        shape = SHAPES[name]
        scale = 1.0 / np.sqrt(shape[1] * shape[2] * shape[3])
        w = (scale * rng.standard_normal(shape)).astype(np.float16)
        P[name] = (w, (0.1 * rng.standard_normal(shape[0])).astype(np.float32))
    return P


def make_inputs(rng, n, ht, wd, round_flow=True):
    """(corr, flow): corr standard normal rounded to float16; flow uniform in [-64, 64] (the reference's clamp),
    float32, holding float16 values with ``round_flow``"""
    corr = rng.standard_normal((n, CORR_PLANES, ht, wd)).astype(np.float16)
    flow = rng.uniform(-FLOW_CLAMP, FLOW_CLAMP, (n, FLOW_PLANES, ht, wd)).astype(np.float32)
    if round_flow:
        flow = flow.astype(np.float16).astype(np.float32)
    return corr, flow


def fixture_inputs(tag):
    """Parameters and inputs of case ``tag`` of tests/golden/ref_encoders.npz, regenerated from the frozen
    ``np.random.RandomState`` stream the generator drew them from: (P, (corr, flow))"""
    rng = np.random.RandomState(FIXTURE_SEED[tag])
    P = make_params(rng)
    return P, make_inputs(rng, *FIXTURE_CASES[tag])


def fixture_case(tag):
    """dict(z: the file, P, corr, flow); loaded once, never modified"""
    if tag not in _fixture:
        P, (corr, flow) = fixture_inputs(tag)
        _fixture[tag] = {"z": np.load(FIXTURE, allow_pickle=False), "P": P, "corr": corr, "flow": flow}
    return _fixture[tag]


GPU_SHAPES = [(2, 3, 5), (3, 9, 17), (2, 8, 16), (1, 48, 64)]   # n x ht x wd of tests/test_gpu_encoders.py
_shape_case = {}


def shape_case(shape):
    """Seeded parameters, inputs and the rounded oracle of both encoders at ``shape`` = (n, ht, wd): dict(P, corr_in,
    flow_in, corr: the corr encoder's dict, flow: the flow encoder's); computed once, never modified"""
    if shape not in _shape_case:
        n, ht, wd = shape
        rng = np.random.default_rng(1000 * n + 10 * ht + wd)
        P = make_params(rng)
        corr, flow = make_inputs(rng, n, ht, wd)
        _shape_case[shape] = {"P": P, "corr_in": corr, "flow_in": flow, "corr": corr_encoder(corr, P),
                              "flow": flow_encoder(flow, P)}
    return _shape_case[shape]


# ---- the whole update operator (tests/golden/ref_update_operator.npz) ----
OP_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_update_operator.npz")
OP_CASES = {"a": (2, 3, 5, [2, 0], True), "b": (1, 4, 6, None, False)}   # n, ht, wd, ii, with flow
OP_SEED = {"a": 20261, "b": 20262}


def op_fixture_inputs(tag):
    """Parameters and inputs of case ``tag`` of ref_update_operator.npz from its frozen stream: (P of the encoders,
    P of the GRU, P of the heads, dict(net, inp, corr, flow or None, ii or None))"""
    import _gru_ref as gr
    n, ht, wd, ii, with_flow = OP_CASES[tag]
    rng = np.random.RandomState(OP_SEED[tag])
    Pe, Pg, Ph = make_params(rng), gr.make_params(rng), hr.make_params(rng)
    net, inp = (rng.standard_normal((n, 128, ht, wd)).astype(np.float16) for _ in range(2))
    corr, flow = make_inputs(rng, n, ht, wd)
    return Pe, Pg, Ph, {"net": net, "inp": inp, "corr": corr, "flow": flow if with_flow else None,
                        "ii": None if ii is None else np.asarray(ii, np.int64)}


def update_operator(net, inp, corr, flow, ii, Pe, Pg, Ph, round16=True, dtype=np.float64):
    """UpdateModule.forward (droid_net.py:120-153) from the three oracles: the corr encoder feeds the GRU's third
    source and the flow encoder its fourth; delta and weight are the heads' first two channels, permuted; eta
    carries the factor 0.01; flow None is zeros.  -> dict(net, delta, weight[, eta, feat])"""
    import _gru_ref as gr
    if flow is None:
        flow = np.zeros((net.shape[0], FLOW_PLANES) + net.shape[2:], np.float32)
    c = corr_encoder(corr, Pe, round16, dtype)["out"]
    f = flow_encoder(flow, Pe, round16, dtype)["out"]
    new = gr.gru(net, inp, c, f, Pg, round16, dtype)["out"]
    h = hr.heads(new, Ph, round16, dtype)
    out = {"net": new, "delta": h["delta"], "weight": h["weight"]}
    if ii is not None:
        uniq, ix = np.unique(ii, return_inverse=True)
        g = hr.graph_agg(new, ix, len(uniq), Ph, round16, dtype)
        out["eta"], out["feat"] = g["eta"], g["feat"]
    return out
