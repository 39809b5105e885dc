"""The float64 oracle of the update operator's output heads (UpdateModule.delta
/ .weight, droid_net.py:102-115, 141-145) and of GraphAgg.forward up to ``eta``
and the features ``upmask`` reads (droid_net.py:65-77), in numpy, with a
per-output error bound.

Parameters ``P``: a dict ``name -> (weight [C_out, 128, 3, 3], bias [C_out])``
with the reference's names ``delta.0``, ``delta.2``, ``weight.0``, ``weight.2``,
``agg.conv1``, ``agg.conv2``, ``agg.eta.0``; the weights hold float16 values.

Rounding points (``round16=True``; they are the kernel's, csrc/droid_conv3x3.hip,
and autocast's): the hidden activations of the heads, the group mean and
``feat`` are rounded to float16 once.  delta, weight and eta are not rounded.
``round16=False`` is the plain float64 evaluation the fixture was recorded with.
``dtype=np.float32`` evaluates the same formulas at the precision of the kernel.

Every value ``v`` comes with two maps of its shape, both derived by first-order
propagation, nothing fitted:

``d``  the most a kernel that follows the contract can differ from ``v``.
       One convolution accumulated in fp32: (K + 2) 2^-24 (sum |w| |x| + |bias|),
       K = 1152 (K products and sums, the bias, one spare).  An input known
       to within dx adds sum |w| dx (a convolution with |w|).  ReLU and the
       mean are 1-Lipschitz; the mean's fp32 sum over c edges and the product
       with 1 / c add (c + 2) 2^-24 mean(|u| + d).  Where both sides round to
       float16 the two roundings may fall on either side of a tie: one ulp16,
       taken at |v| + d.  sigmoid has slope <= 1/4, softplus <= 1; their fp32
       evaluation (expf, log1pf: 2 ulp each, the sum, the quotient or the
       product with 0.01f) adds 8 x 2^-24 |v|.
``r``  the most ``v`` (float16 rounding points in) differs from the plain
       float64 value: half an ulp16 at each rounding point, pushed through the
       later layers the same way.

So |kernel - oracle| <= d, and |kernel - recorded float64 reference| <= d + r.
"""
from __future__ import annotations

import os

import numpy as np

from _upsample_ref import round_fp16, ulp_fp16

K = 9 * 128
U32 = 2.0 ** -24
NAMES = ("delta.0", "delta.2", "weight.0", "weight.2", "agg.conv1", "agg.conv2", "agg.eta.0")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_update_heads.npz")
_fixture = {}


def conv3x3(x, w, b=None):
    """x [n, C, ht, wd], w [C_out, C, 3, 3], b [C_out] or None -> [n, C_out, ht, wd]; padding 1, in x's dtype"""
    n, C, ht, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    w = w.astype(x.dtype)
    out = np.zeros((n, w.shape[0], ht * wd), x.dtype)
    for ky in range(3):
        for kx in range(3):
            out += np.matmul(w[:, :, ky, kx], xp[:, :, ky:ky + ht, kx:kx + wd].reshape(n, C, ht * wd))
    if b is not None:
        out += b.astype(x.dtype)[None, :, None]
    return out.reshape(n, -1, ht, wd)


def conv_layer(x, w, b, dx=None, rx=None, dtype=np.float64):
    """One convolution of x (known to the kernel within dx, off the plain
    float64 value by at most rx) -> (v, d, r) before any activation."""
    x64 = np.asarray(x, np.float64)
    w64, b64 = np.asarray(w, np.float64), np.asarray(b, np.float64)
    v = conv3x3(x64.astype(dtype), w64, b64).astype(np.float64)
    n = x64.shape[0]
    a = conv3x3(np.concatenate([np.abs(x64)] + [m for m in (dx, rx) if m is not None]), np.abs(w64))
    d = (K + 2) * U32 * (a[:n] + np.abs(b64)[None, :, None, None])
    if dx is not None:
        d = d + a[n:2 * n]
    r = np.zeros_like(v) if rx is None else a[-n:]
    return v, d, r


def relu_store16(v, d, r, round16=True):
    """ReLU, then the float16 rounding point of an activation that goes to memory"""
    u = np.maximum(v, 0.0)
    if not round16:
        return u, d, r
    return round_fp16(u), d + ulp_fp16(u + d), r + 0.5 * ulp_fp16(u)


def conv_relu(x, w, b, round16=True, dtype=np.float64):
    """fp16(ReLU(conv(x) + b)) of an exactly known x -> (value, d)"""
    v, d, r = conv_layer(x, w, b, dtype=dtype)
    out, d, _ = relu_store16(v, d, r, round16)
    return out, d


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def softplus(v):
    return np.where(v > 20.0, v, np.log1p(np.exp(np.minimum(v, 20.0))))


def heads(net, P, round16=True, dtype=np.float64):
    """net [n, 128, ht, wd] -> dict(hidden [n, 256, ht, wd] (delta.0 over
    weight.0), delta, weight [n, ht, wd, 2]) and d_* / r_* of each"""
    w0 = np.concatenate([P["delta.0"][0], P["weight.0"][0]])
    b0 = np.concatenate([P["delta.0"][1], P["weight.0"][1]])
    hid, dh, rh = relu_store16(*conv_layer(net, w0, b0, dtype=dtype), round16)
    out = {"hidden": hid, "d_hidden": dh, "r_hidden": rh}
    for name, lo in (("delta", 0), ("weight", 128)):
        w, b = P[name + ".2"]
        v, d, r = conv_layer(hid[:, lo:lo + 128], w, b, dh[:, lo:lo + 128], rh[:, lo:lo + 128], dtype)
        if name == "weight":
            v = sigmoid(v)
            d, r = 0.25 * d + 8 * U32 * v, 0.25 * r
        for key, m in ((name, v), ("d_" + name, d), ("r_" + name, r)):
            out[key] = np.ascontiguousarray(m.transpose(0, 2, 3, 1))
    return out


def graph_agg(net, ix, G, P, round16=True, dtype=np.float64):
    """net [n, 128, ht, wd], ix [n] in [0, G) -> dict(mean, feat [G, 128, ht,
    wd], eta [G, ht, wd]) and d_* / r_* of each; an empty group has mean zero"""
    ix = np.asarray(ix, np.int64)
    v, d, r = conv_layer(net, *P["agg.conv1"], dtype=dtype)
    u = np.maximum(v, 0.0)
    shape = (G,) + u.shape[1:]
    mean, dm, rm = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for g in range(G):
        sel = np.flatnonzero(ix == g)
        c = len(sel)
        if c == 0:
            continue
        if dtype == np.float32:  # the kernel's order: ascending edges, x 1 / c
            acc = np.zeros(shape[1:], np.float32)
            for e in sel:
                acc = acc + u[e].astype(np.float32)
            mean[g] = (acc * np.float32(1.0 / c)).astype(np.float64)
        else:
            mean[g] = u[sel].mean(axis=0)
        dm[g] = d[sel].mean(axis=0)
        dm[g] += (c + 2) * U32 * (mean[g] + dm[g])
        rm[g] = r[sel].mean(axis=0)
    if round16:
        dm, rm = dm + ulp_fp16(mean + dm), rm + 0.5 * ulp_fp16(mean)
        mean = round_fp16(mean)
    feat, df, rf = relu_store16(*conv_layer(mean, *P["agg.conv2"], dm, rm, dtype), round16)
    ve, de, re = conv_layer(feat, *P["agg.eta.0"], df, rf, dtype)
    eta = 0.01 * softplus(ve)
    return {"mean": mean, "d_mean": dm, "r_mean": rm, "feat": feat, "d_feat": df, "r_feat": rf,
            "eta": eta[:, 0], "d_eta": (0.01 * de + 8 * U32 * eta)[:, 0], "r_eta": 0.01 * re[:, 0]}


def make_params(rng, scale=None):
    """Seeded parameters with float16 weight values scaled by 1 / sqrt(1152), so
    activations stay O(1) and about half the ReLUs are active."""
    scale = 1.0 / np.sqrt(K) if scale is None else scale
    P = {}
    for name in NAMES:
        c_out = {"delta.2": 2, "weight.2": 2, "agg.eta.0": 1}.get(name, 128)
        w = (scale * rng.standard_normal((c_out, 128, 3, 3))).astype(np.float16)
        b = (0.1 * rng.standard_normal(c_out)).astype(np.float32)
        P[name] = (w, b)
    return P


def fixture_case(tag):
    """Case ``tag`` of tests/golden/ref_update_heads.npz: dict(z: the file, P: its
    parameters and net: its input, the stored input-channel slices put back
    among zeros, ix, G: the groups of its ii); loaded once, never modified."""
    if tag not in _fixture:
        z = np.load(FIXTURE, allow_pickle=False)
        P = {}
        for name in NAMES:
            key = name.replace(".", "_")
            w = z[key + "_w"]
            full = np.zeros((w.shape[0], 128, 3, 3), np.float16)
            full[:, :w.shape[1]] = w
            P[name] = (full, z[key + "_b"])
        live = z[f"{tag}_net"]
        net = np.zeros((live.shape[0], 128) + live.shape[2:], np.float16)
        net[:, :live.shape[1]] = live
        uniq, ix = np.unique(z[f"{tag}_ii"], return_inverse=True)
        _fixture[tag] = {"z": z, "P": P, "net": net, "ix": ix, "G": len(uniq)}
    return _fixture[tag]
