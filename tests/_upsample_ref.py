"""The float64 oracle of the convex upsampling (cvx_upsample, droid_net.py:23-37)
and of the mask head (GraphAgg.upmask, a 1 x 1 convolution 576 <- C), in numpy.

With pad the zero-padded map,

    up[n, 8y+a, 8x+b, c] = sum_{k=0..8} softmax_k(mask[n, 64k + 8a + b, y, x])
                                        * pad[n, y + k//3 - 1, x + k%3 - 1, c]

``cvx_upsample(data, mask, dtype)`` evaluates it in ``dtype`` (float64: the
oracle; float32: the same formula at the precision of the kernel, from which
the GPU tests derive their bound) and returns, per output element,

    mag    = sum_k w_k |d_k|                     the magnitude the error scales with
    spread = max_k d_k - min_k d_k               over the nine neighbours, padding zeros included

``head`` gives the logits as the reference computes them under autocast: the
exact (float64) dot product plus bias, rounded once to float16.
"""
from __future__ import annotations

import numpy as np

MASK_CHANNELS = 576


def round_fp16(x):
    return np.asarray(x).astype(np.float16).astype(np.float64)


def ulp_fp16(x):
    """The spacing of float16 at |x| (2^-24 below the smallest normal)."""
    ax = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(ax)) - 10)


def neighbours(data):
    """data [n, ht, wd, dim] -> [n, 9, ht, wd, dim]: neighbour k = (k // 3 - 1, k % 3 - 1) of the zero-padded map"""
    n, ht, wd, dim = data.shape
    pad = np.pad(data, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return np.stack([pad[:, k // 3:k // 3 + ht, k % 3:k % 3 + wd] for k in range(9)], axis=1)


def _fine(a):
    """[n, 8 (a), 8 (b), ht, wd, dim] -> [n, 8 ht, 8 wd, dim]"""
    n, _, _, ht, wd, dim = a.shape
    return np.ascontiguousarray(a.transpose(0, 3, 1, 4, 2, 5)).reshape(n, 8 * ht, 8 * wd, dim)


def cvx_upsample(data, mask, dtype=np.float64):
    """data [n, ht, wd, dim], mask n x 576 x ht x wd values -> dict(up, mag, spread), each [n, 8 ht, 8 wd, dim]"""
    data = np.asarray(data).astype(dtype)
    n, ht, wd, dim = data.shape
    m = np.asarray(mask).astype(dtype).reshape(n, 9, 8, 8, ht, wd)
    e = np.exp(m - m.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True)                      # [n, 9, 8, 8, ht, wd]
    d = neighbours(data)[:, :, None, None]                    # [n, 9, 1, 1, ht, wd, dim]
    up = (w[..., None] * d).sum(axis=1)
    mag = (w[..., None] * np.abs(d)).sum(axis=1)
    spread = np.broadcast_to(d.max(axis=1) - d.min(axis=1), up.shape)
    return {"up": _fine(up), "mag": _fine(mag), "spread": _fine(spread)}


def head(feat, weight, bias):
    """feat [n, C, ht, wd], weight [576, C] (or [576, C, 1, 1]), bias [576] -> dict(
    logits: float16-rounded [n, 576, ht, wd] (as float64), exact: before the
    rounding, absdot: sum_c |w| |f| + |bias|)"""
    f = np.asarray(feat, np.float64)
    w = np.asarray(weight, np.float64).reshape(MASK_CHANNELS, -1)
    b = np.asarray(bias, np.float64).reshape(MASK_CHANNELS)
    n, C, ht, wd = f.shape
    flat = f.reshape(n, C, ht * wd)
    exact = (np.matmul(w, flat) + b[None, :, None]).reshape(n, MASK_CHANNELS, ht, wd)
    absdot = (np.matmul(np.abs(w), np.abs(flat)) + np.abs(b)[None, :, None]).reshape(n, MASK_CHANNELS, ht, wd)
    return {"logits": round_fp16(exact), "exact": exact, "absdot": absdot}


def logit_delta(h, C):
    """The most a logit formed as an fp32 sum over C, + bias in fp32, one
    rounding to float16, can differ from the exact logit ``h['exact']``: the
    fp32 part s = (C + 2) 2^-24 (sum |w| |f| + |bias|), plus half a float16 ulp
    (taken at |exact| + s, where the rounded value may lie)."""
    s = (C + 2) * 2.0 ** -24 * h["absdot"]
    return 0.5 * ulp_fp16(np.abs(h["exact"]) + s) + s


def perturbation_bound(delta, spread):
    """A perturbation of every logit of a (pixel, a, b) by at most d = max_k
    delta_k moves the convex combination by at most (e^{2d} - 1) spread / 2.
    (Moving the logits by e_k in [-d, d] multiplies the weights by e^{e_k} and
    renormalises; the combination moves by at most spread x the total
    variation between the two weight vectors, which is at most tanh(d / 2):
    mass p moved up and 1 - p moved down, at the worst p = 1 / (1 + e^d).
    tanh(d) <= d <= (e^{2d} - 1) / 2, so
    the bound also holds between two sets of logits that are each within d of
    the exact ones, 2d apart: the kernel's and the oracle's rounded logits.)
    delta [n, 576, ht, wd], spread [n, 8 ht, 8 wd, dim] -> [n, 8 ht, 8 wd, dim]"""
    n, _, ht, wd = delta.shape
    dmax = delta.reshape(n, 9, 8, 8, ht, wd).max(axis=1)[..., None]   # [n, 8, 8, ht, wd, 1]
    dmax = _fine(dmax)
    return np.expm1(2.0 * dmax) * spread / 2.0
