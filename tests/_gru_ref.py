"""The float64 oracle of the update operator's ConvGRU (gru.py:34-48, called at
droid_net.py:138 as ``self.gru(net, inp, corr, flow)``), in numpy, with a
per-output error bound:

    glo  = mean over an edge's pixels of sigmoid(w(net)) * net                   [n, 128]
    gbias[:, 128 k + co] = b_k[co] + (W_k_glo glo)[co] + b_k_glo[co]             k = z, r, q
    z    = sigmoid(convz([net, inp, corr, flow]) + gbias_z)
    rnet = sigmoid(convr([net, inp, corr, flow]) + gbias_r) * net
    net' = (1 - z) net + z tanh(convq([rnet, inp, corr, flow]) + gbias_q)

Parameters ``P``: a dict ``name -> (weight, bias)`` with the reference's names
``convz``, ``convr``, ``convq`` ([128, 448, 3, 3]), ``w``, ``convz_glo``,
``convr_glo``, ``convq_glo`` ([128, 128, 1, 1]); the weights hold float16 values,
the biases float32 values.

Rounding points (``round16=True``; they are the kernel's, csrc/droid_gru.hip):
``z``, ``rnet`` and ``net'`` are rounded to float16 once each; everything else,
``gbias`` included, is never rounded to float16.  ``round16=False`` is the plain
float64 evaluation the fixture was recorded with.  ``dtype=np.float32``
evaluates the same formulas at the precision of the kernel, the activations by
the kernel's own expressions (below).

Every value ``v`` comes with two maps of its shape, both derived by first-order
propagation, nothing fitted (u = 2^-24, the relative error of one fp32 rounding):

``d``  the most a kernel that follows the contract can differ from ``v``.
       A sum of K products accumulated in fp32, plus its bias: (K + 2) u (sum
       |w| |x| + |bias|); K = 9 x 448 = 4032 for the three convolutions, 128 for
       ``w`` and (with two biases, K + 3) for the glo products.  An input known
       to within dx adds sum |w| dx.  The mean over HW pixels, an fp32 sum in
       any order and the product with 1 / HW: (HW + 2) u mean |t| on top of the
       mean of the terms' own bounds.  sigmoid has slope <= 1/4, tanh <= 1.  A
       product a b: |b| da + |a| db and one rounding u |a b|.  The blend
       (1 - z) h + z q with h exact: |q - h| dz + (|z| + dz) dq, and four fp32
       operations, 4 u (|h| + |q|).  Where both sides round to float16 the two
       roundings may fall on either side of a tie: one ulp16, taken at |v| + d.

       The activations in fp32, from the expressions the kernel uses.  expf is
       taken as exact to 2 ulp = 4 u relative, a quotient to 2.5 ulp = 5 u, a
       sum or difference to u.
         sigmoid(v) = 1 / (1 + expf(-v)): with e = exp(-v) the denominator 1 + e
           has relative error 4 u e / (1 + e) + u <= 5 u, the quotient 5 u more:
           10 u relative, and the value is at most 1: SIG_ABS = 12 u absolute.
         tanh(v) = 1 - 2 / (1 + expf(2 v)): 2 v is exact; t = 2 / (1 + e) has
           relative error <= 10 u as above and t <= 2: 20 u absolute; the
           difference 1 - t, at most 1 in magnitude, rounds with u more: 21 u;
           TANH_ABS = 24 u absolute.  (Near v = 0 the difference cancels: the
           bound is absolute, as the contract's is.)  expf overflowing to
           infinity gives exactly 1, underflowing to 0 exactly -1.
``r``  the most ``v`` (float16 rounding points in) differs from the plain
       float64 value: half an ulp16 at each rounding point, pushed through the
       later stages the same way.  ``gbias`` has no rounding point before it: r = 0.

So |kernel - oracle| <= d, and |kernel - recorded float64 reference| <= d + r.

The stage functions take their inputs as arguments, so that a stage can be
evaluated on the kernel's own intermediates (exactly known values: no dx).
"""
from __future__ import annotations

import os

import numpy as np

from _upsample_ref import round_fp16, ulp_fp16

C = 128
CIN = 3 * C + C // 2
K = 9 * CIN
U32 = 2.0 ** -24
SIG_ABS = 12 * U32
TANH_ABS = 24 * U32
NAMES = ("convz", "convr", "convq", "w", "convz_glo", "convr_glo", "convq_glo")
GATES = ("convz", "convr", "convq")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_gru.npz")
FIXTURE_CASES = {"a": (2, 3, 5), "b": (1, 6, 18)}
FIXTURE_SEED = {"a": 20241, "b": 20242}
FIXTURE_ZR_ROWS = slice(0, C, 2)   # z and rnet are recorded for the even channels (the file's size), net' for all
_fixture = {}


def conv3x3(x, w):
    """x [n, C, ht, wd], w [C_out, C, 3, 3] -> [n, C_out, ht, wd]; padding 1, no bias, in x's dtype (each tap one
    contiguous matrix product)"""
    n, C, ht, wd = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    w = w.astype(x.dtype)
    out = np.zeros((n, w.shape[0], ht * wd), x.dtype)
    for ky in range(3):
        for kx in range(3):
            tap = np.ascontiguousarray(w[:, :, ky, kx])
            for e in range(n):
                out[e] += tap @ np.ascontiguousarray(xp[e, :, ky:ky + ht, kx:kx + wd]).reshape(C, ht * wd)
    return out.reshape(n, -1, ht, wd)


def sigmoid(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def tanh(v):
    """np.tanh in float64; in float32 the kernel's 1 - 2 / (1 + exp(2 v))"""
    if v.dtype == np.float32:
        with np.errstate(over="ignore"):
            return np.float32(1) - np.float32(2) / (np.float32(1) + np.exp(np.float32(2) * v))
    return np.tanh(v)


def _mat(P, name):
    w, b = P[name]
    return np.asarray(w, np.float64).reshape(C, C), np.asarray(b, np.float64)


def glo_bias(net, P, dtype=np.float64):
    """net [n, 128, ht, wd] -> (gbias [n, 384], d, r = 0)"""
    n = net.shape[0]
    x = np.asarray(net, np.float64).reshape(n, C, -1)
    HW = x.shape[2]
    ww, wb = _mat(P, "w")
    a = (np.matmul(ww.astype(dtype), x.astype(dtype)) + wb.astype(dtype)[None, :, None])
    da = (C + 2) * U32 * (np.matmul(np.abs(ww), np.abs(x)) + np.abs(wb)[None, :, None])
    s = sigmoid(a)
    ds = 0.25 * da + SIG_ABS
    u = s * x.astype(dtype)
    du = np.abs(x) * ds + U32 * np.abs(u)
    if dtype == np.float32:
        glo = (u.sum(axis=2, dtype=np.float32) * np.float32(1.0 / HW))
    else:
        glo = u.mean(axis=2)
    dglo = du.mean(axis=2) + (HW + 2) * U32 * np.abs(u).astype(np.float64).mean(axis=2)
    out, d = [], []
    for name in GATES:
        wg, bg = _mat(P, name + "_glo")
        bk = np.asarray(P[name][1], np.float64)
        v = bk.astype(dtype)[None] + np.matmul(glo, wg.astype(dtype).T) + bg.astype(dtype)[None]
        g64 = np.abs(glo).astype(np.float64)
        out.append(v.astype(np.float64))
        d.append((C + 3) * U32 * (np.matmul(g64, np.abs(wg).T) + np.abs(bk)[None] + np.abs(bg)[None])
                 + np.matmul(dglo, np.abs(wg).T))
    gb = np.concatenate(out, axis=1)
    return gb, np.concatenate(d, axis=1), np.zeros_like(gb)


def _gate(x, w, gb, dgb, dx, rx, dtype):
    """conv(x) + gbias before the activation: x [n, 448, ht, wd] float64 of which the first 128 channels are
    known to the kernel within dx and off the plain value by at most rx (or None) -> (v, d, r)"""
    w64 = np.asarray(w, np.float64)
    v = (conv3x3(x.astype(dtype), w64) + gb.astype(dtype)[:, :, None, None]).astype(np.float64)
    d = (K + 2) * U32 * (conv3x3(np.abs(x), np.abs(w64)) + np.abs(gb)[:, :, None, None])
    if dgb is not None:
        d = d + dgb[:, :, None, None]
    r = np.zeros_like(v)
    if dx is not None:
        d = d + conv3x3(dx, np.abs(w64[:, :C]))
    if rx is not None:
        r = conv3x3(rx, np.abs(w64[:, :C]))
    return v, d, r


def _store16(v, d, r, round16):
    if not round16:
        return v, d, r
    return round_fp16(v), d + ulp_fp16(np.abs(v) + d), r + 0.5 * ulp_fp16(v)


def _f64(*maps):
    return [np.asarray(m, np.float64) for m in maps]


def stage_zr(net, inp, corr, flow, gbias, P, dgb=None, round16=True, dtype=np.float64):
    """The zr launch on exactly known activations and a gbias known within dgb ->
    dict(z, rnet) with d_* and r_*"""
    net, inp, corr, flow, gbias = _f64(net, inp, corr, flow, gbias)
    x = np.concatenate([net, inp, corr, flow], axis=1)
    w = np.concatenate([P["convz"][0], P["convr"][0]])
    v, d, r = _gate(x, w, gbias[:, :2 * C], None if dgb is None else dgb[:, :2 * C], None, None, dtype)
    s = sigmoid(v.astype(dtype)).astype(np.float64)
    ds = 0.25 * d + SIG_ABS
    z, dz, rz = _store16(s[:, :C], ds[:, :C], r[:, :C], round16)
    rn = (s[:, C:].astype(dtype) * net.astype(dtype)).astype(np.float64)
    drn = np.abs(net) * ds[:, C:] + U32 * np.abs(rn)
    rn, drn, rrn = _store16(rn, drn, np.abs(net) * r[:, C:], round16)
    return {"z": z, "d_z": dz, "r_z": rz, "rnet": rn, "d_rnet": drn, "r_rnet": rrn}


def stage_q(rnet, inp, corr, flow, gbias, z, net, P, d_rnet=None, r_rnet=None, dgb=None, d_z=None, r_z=None,
            round16=True, dtype=np.float64):
    """The q launch -> dict(out, d_out, r_out); rnet, gbias and z exactly known unless their d / r are given"""
    rnet, inp, corr, flow, gbias, z, net = _f64(rnet, inp, corr, flow, gbias, z, net)
    x = np.concatenate([rnet, inp, corr, flow], axis=1)
    v, d, r = _gate(x, P["convq"][0], gbias[:, 2 * C:], None if dgb is None else dgb[:, 2 * C:], d_rnet, r_rnet,
                    dtype)
    q = tanh(v.astype(dtype)).astype(np.float64)
    dq = d + TANH_ABS
    t = dtype
    out = ((np.asarray(1, t) - z.astype(t)) * net.astype(t) + z.astype(t) * q.astype(t)).astype(np.float64)
    dz = np.zeros_like(z) if d_z is None else d_z
    rz = np.zeros_like(z) if r_z is None else r_z
    do = np.abs(q - net) * dz + (np.abs(z) + dz) * dq + 4 * U32 * (np.abs(net) + np.abs(q))
    ro = np.abs(q - net) * rz + (np.abs(z) + rz) * r
    out, do, ro = _store16(out, do, ro, round16)
    return {"out": out, "d_out": do, "r_out": ro, "q": q}


def gru(net, inp, corr, flow, P, round16=True, dtype=np.float64):
    """End to end -> dict(gbias, z, rnet, out) with d_* and r_* of each"""
    gb, dgb, rgb = glo_bias(net, P, dtype)
    zr = stage_zr(net, inp, corr, flow, gb, P, dgb, round16, dtype)
    q = stage_q(zr["rnet"], inp, corr, flow, gb, zr["z"], net, P, zr["d_rnet"], zr["r_rnet"], dgb, zr["d_z"],
                zr["r_z"], round16, dtype)
    return {"gbias": gb, "d_gbias": dgb, "r_gbias": rgb, **zr, **{k: q[k] for k in ("out", "d_out", "r_out")}}


def make_params(rng, scale3=None, scale1=None):
    """Seeded parameters (``rng``: a Generator or a RandomState) with float16 weight values, the 3 x 3 ones
    scaled by 1 / sqrt(4032) and the 1 x 1 ones by 1 / sqrt(128), so that the gates stay O(1)."""
    scale3 = 1.0 / np.sqrt(K) if scale3 is None else scale3
    scale1 = 1.0 / np.sqrt(C) if scale1 is None else scale1
    P = {}
    for name in NAMES:
        if name in GATES:
            w = (scale3 * rng.standard_normal((C, CIN, 3, 3))).astype(np.float16)
        else:
            w = (scale1 * rng.standard_normal((C, C, 1, 1))).astype(np.float16)
        P[name] = (w, (0.1 * rng.standard_normal(C)).astype(np.float32))
    return P


def make_inputs(rng, n, ht, wd):
    """(net, inp, corr, flow): standard normal rounded to float16"""
    return tuple(rng.standard_normal((n, c, ht, wd)).astype(np.float16) for c in (C, C, C, C // 2))


def fixture_inputs(tag):
    """Parameters and inputs of case ``tag`` of tests/golden/ref_gru.npz, regenerated from the frozen
    ``np.random.RandomState`` stream the generator drew them from: (P, (net, inp, corr, flow))"""
    rng = np.random.RandomState(FIXTURE_SEED[tag])
    P = make_params(rng)
    return P, make_inputs(rng, *FIXTURE_CASES[tag])


def fixture_case(tag):
    """dict(z: the file, P, net, inp, corr, flow); loaded once, never modified"""
    if tag not in _fixture:
        P, (net, inp, corr, flow) = fixture_inputs(tag)
        _fixture[tag] = {"z": np.load(FIXTURE, allow_pickle=False), "P": P, "net": net, "inp": inp, "corr": corr,
                         "flow": flow}
    return _fixture[tag]
