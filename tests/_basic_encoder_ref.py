"""The float64 oracle of the tracker's feature and context encoders
(DroidNet.fnet / .cnet, the BasicEncoder of extractor.py:75-141), in numpy
(the convolutions by torch on the CPU, float64), launch by launch as csrc/droid_basic_encoder.hip computes them:

    stem    Conv 7 x 7 stride 2, 3 -> 32; N; ReLU
    layer1  2 x block(32 -> 32); layer2  block(32 -> 64, stride 2), block(64 -> 64)
    layer3  block(64 -> 128, stride 2), block(128 -> 128); head  Conv 1 x 1, 128 -> out
    block(x) = ReLU(x' + ReLU(N(conv2(ReLU(N(conv1(x))))))), x' = N(Conv 1 x 1 stride 2 (x)) at stride 2, else x

N is an instance norm without parameters (biased variance, eps 1e-5; ``norm =
"instance"``, fnet, out = 128) or the identity (``"none"``, cnet, out = 256, split
into net = tanh(rows 0 .. 127) and inp = relu(rows 128 .. 255)).  Padding k // 2,
so a stride-2 output is ceil(in / 2) pixels.

Parameters ``P``: a dict ``name -> (weight, bias)`` with the module's names
(``conv1``, ``layer1.0.conv1`` .. ``layer3.1.conv2``, ``layer2.0.downsample.0``,
``layer3.0.downsample.0``, ``conv2``); the weights hold float16 values, the
biases float32 values, the image float16 values (the kernel rounds the
normalised image to float16 as it reads it).

Rounding contract (``round16=True``): one rounding to float16 per stored raw map
R = conv + bias; one per staged operand, taken over the whole expression

    A  ReLU(N(R))      B  ReLU(P + ReLU(N(R)))      C  ReLU(N(Rd) + ReLU(N(R)))

evaluated in fp32; one for the result.  The statistics of N are those of the
stored (rounded) map.  ``round16=False`` is the plain float64 evaluation.

One function per launch (``stem``, ``stage`` + ``conv``, ``head``, ``stats``).
Each takes the *stored* inputs of its launch (float16 maps, float32 statistics)
and returns the value with a bound ``d`` on what a kernel that follows the
contract may differ by, derived, nothing fitted:

* the fp32 accumulation of K products and the bias: (K + 2) 2^-24 (sum |w| |a| + |b|);
* one ulp16 for the rounding of the stored output, taken at |v| + d;
* a staged operand is evaluated in fp32 from exactly known inputs: a
  subtraction, a product, the same for the second term, a sum (contracted or
  not): at most 4 2^-24 (|N(R)| + |second term|) off the float64 value, so both
  sides round to the same float16 unless the float64 value lies within that of
  a rounding tie, where they may differ by one ulp16: ``d`` of the operand is
  one ulp16 there and zero elsewhere;
* that ``d`` pushed through the convolution as sum |w| d.

``encoder`` chains the launches (the statistics taken in float64 from its own
stored maps) and, with ``round16``, carries ``r``: a first-order bound on the
rounded evaluation's distance from the plain one (half an ulp16 per rounding
point, pushed through the convolutions as sum |w| r and through N by the
change it allows in the mean and the standard deviation).  After 14 layers ``r``
is far above what happens; the end-to-end check of the GPU tests is the rms
ratio E16 described there.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from _upsample_ref import round_fp16, ulp_fp16  # noqa: F401  (re-exported)

U32 = 2.0 ** -24
EPS = 1e-5
DIMS = (32, 64, 128)
OUT = {"instance": 128, "none": 256}
BLOCKS = ("layer1.0", "layer1.1", "layer2.0", "layer2.1", "layer3.0", "layer3.1")
CNET_HEAD_SCALE = 1.0 / 12   # the cnet head's weights, scaled so that its pre-activation rms lies in [0.5, 2]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_basic_encoder.npz")
FIXTURE_CASES = {"f": ("instance", 1, 16, 24), "c": ("none", 1, 21, 27)}
FIXTURE_SEED = {"f": 20271, "c": 20272}
FIXTURE_EVEN = slice(0, None, 2)             # the hooked maps are recorded for the even channels (the file's size)
GPU_SHAPES = [(2, 16, 24), (1, 37, 53), (3, 64, 128), (1, 72, 136)]   # n x H x W of tests/test_gpu_basic_encoder.py
_fixture, _shape_case = {}, {}


def param_shapes(norm):
    shapes = {"conv1": (DIMS[0], 3, 7, 7)}
    c_in = DIMS[0]
    for name in BLOCKS:
        c_out = DIMS[int(name[5]) - 1]
        shapes[f"{name}.conv1"] = (c_out, c_in, 3, 3)
        shapes[f"{name}.conv2"] = (c_out, c_out, 3, 3)
        if c_out != c_in:
            shapes[f"{name}.downsample.0"] = (c_out, c_in, 1, 1)
        c_in = c_out
    shapes["conv2"] = (OUT[norm], DIMS[2], 1, 1)
    return shapes


def make_params(rng, norm):
    """Seeded parameters: float16 weight values normal x sqrt(2 / K) (K = C_in k k), biases 0.1 x normal; the cnet
    head scaled by CNET_HEAD_SCALE (without a norm the residual sums grow from block to block), which keeps tanh
    off saturation"""
    P = {}
    for name, shape in param_shapes(norm).items():
        scale = np.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        if name == "conv2" and norm == "none":
            scale *= CNET_HEAD_SCALE
        w = (scale * rng.standard_normal(shape)).astype(np.float16)
        P[name] = (w, (0.1 * rng.standard_normal(shape[0])).astype(np.float32))
    return P


def make_images(rng, n, H, W):
    """[n, 3, H, W] float32 holding float16 values: standard normal, what a normalised image looks like"""
    return rng.standard_normal((n, 3, H, W)).astype(np.float16).astype(np.float32)


def sizes(H, W):
    out = []
    for _ in range(3):
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return out


def conv2d(x, w, b=None, stride=1):
    """x [n, C, h, w], w [C_out, C, k, k] (k odd), b [C_out] or None -> [n, C_out, ceil(h / stride), ceil(w / stride)];
    padding k // 2; float64 (torch's CPU convolution: the GPU tests evaluate a few hundred of them)"""
    t = lambda m: torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64))  # noqa: E731
    out = F.conv2d(t(x), t(w), None if b is None else t(b), stride, np.shape(w)[2] // 2)
    return out.numpy()


def _store(v, d, round16):
    if not round16:
        return v, d
    return round_fp16(v), d + ulp_fp16(np.abs(v) + d)


def _conv(a, da, w, b, stride, round16):
    """the raw map of one convolution of the staged operand a (known to the kernel within da) -> (R, d)"""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    v = conv2d(a, w, b, stride)
    mag = conv2d(np.abs(a), np.abs(w), np.abs(b), stride)
    d = (K + 2) * U32 * mag
    if da is not None and da.any():
        d = d + conv2d(da, np.abs(w), None, stride)
    return _store(v, d, round16)


def stem(images, w, b, round16=True):
    """Launch 1: images [n, 3, H, W] (float16 values) -> (R0, d)"""
    return _conv(np.asarray(images, np.float64), None, w, b, 2, round16)


def normalise_image(images, mean, std):
    """what the stem reads with mean / std: fp16((x - mean_c) / std_c), the arithmetic in float32"""
    x = np.asarray(images, np.float32)
    m, s = (np.asarray(v, np.float32).reshape(1, 3, 1, 1) for v in (mean, std))
    return ((x - m) / s).astype(np.float16).astype(np.float32)


def stats(R, parts=1):
    """(mean, rstd, d_mean, d_rstd) [n, C] of a stored map R [n, C, h, w] in float64, with the bound of the kernel's
    fp32 evaluation: two-pass partials over at most 32 values, merged with Chan's formula in a chain of at most L =
    ceil(parts / 64) + 6 merges (``parts``: wgsr_droid_be_parts of the map).  Mean: a 32-term sum and a division, (32
    + 2) u, then per merge a subtraction, a ratio, a product and a sum on values no larger than max |R|, 4 u each.
    M2: every term is non-negative, so the errors stay relative: (32 + 4) u for a partial, 6 u per merge; an error
    e in the partial means moves the between-partial term by at most 2 sqrt(var) e + e^2.  rstd = (var + eps)^-1/2:
    its derivative 0.5 rstd^3 at the ends of the interval, and 4 u rstd for the division, the sum, the root and the
    reciprocal."""
    R = np.asarray(R, np.float64)
    L = -(-parts // 64) + 6
    mean = R.mean(axis=(2, 3))
    var = R.var(axis=(2, 3))
    rstd = 1.0 / np.sqrt(var + EPS)
    top = np.abs(R).max(axis=(2, 3))
    d_mean = (34 + 4 * L) * U32 * top
    d_var = (36 + 6 * L) * U32 * var + 2 * np.sqrt(var) * d_mean + d_mean ** 2
    lo = 1.0 / np.sqrt(np.maximum(var - d_var, 0.0) + EPS)
    hi = 1.0 / np.sqrt(var + d_var + EPS)
    d_rstd = np.maximum(lo - rstd, rstd - hi) + 4 * U32 * lo
    return mean, rstd, d_mean, d_rstd


def _norm(R, st):
    if st is None:
        return np.asarray(R, np.float64)
    mean, rstd = (np.asarray(v, np.float64)[:, :, None, None] for v in st)
    return (np.asarray(R, np.float64) - mean) * rstd


def stage(R, st, P=None, pst=None, round16=True):
    """The staged operand of a launch from its stored inputs: form A (P None), B (pst None) or C -> (a, d); also the
    side output.  st / pst: (mean, rstd) [n, C] each, or None for the identity."""
    a = np.maximum(_norm(R, st), 0.0)
    mag = a.copy()
    if P is not None:
        second = _norm(P, pst)
        mag = mag + np.abs(second)
        a = np.maximum(second + a, 0.0)
    if not round16:
        return a, np.zeros_like(a)
    a16 = np.asarray(a).astype(np.float16)
    lo = np.nextafter(a16, np.float16(-np.inf)).astype(np.float64)
    hi = np.nextafter(a16, np.float16(np.inf)).astype(np.float64)
    v16 = a16.astype(np.float64)
    gap = np.minimum(np.abs(a - 0.5 * (v16 + lo)), np.abs(a - 0.5 * (v16 + hi)))
    d = np.where(gap <= 4 * U32 * mag, np.maximum(v16 - lo, hi - v16), 0.0)
    return v16, d


def conv(a, da, w3, b3, stride=1, w1=None, b1=None, round16=True):
    """A convolution launch on the staged operand: the 3 x 3 rows and, stacked under them, the 1 x 1 rows that read
    the centre tap (the downsample at stride 2) -> (R [n, rows3 + rows1, ho, wo], d)"""
    R, d = _conv(a, da, w3, b3, stride, round16)
    if w1 is not None:
        Rd, dd = _conv(a, da, w1, b1, stride, round16)
        R, d = np.concatenate([R, Rd], axis=1), np.concatenate([d, dd], axis=1)
    return R, d


def head(a, da, w, b, norm, round16=True):
    """The 1 x 1 head: fnet -> (out, d); cnet -> ((net, inp), (d_net, d_inp)).  tanh and ReLU are 1-Lipschitz; the
    kernel's fp32 tanh adds 4 2^-24 (a few ulp32 of a value below 1)."""
    K = w.shape[1]
    v = conv2d(a, w, b)
    d = (K + 2) * U32 * conv2d(np.abs(a), np.abs(w), np.abs(b))
    if da is not None and da.any():
        d = d + conv2d(da, np.abs(w))
    if norm == "instance":
        return _store(v, d, round16)
    net, d_net = _store(np.tanh(v[:, :128]), d[:, :128] + 4 * U32, round16)
    inp, d_inp = _store(np.maximum(v[:, 128:], 0.0), d[:, 128:], round16)
    return (net, inp), (d_net, d_inp)


# the launches after the stem: name, the raw map(s) it reads as R, the second term ("X3": a block output, "Rd5": a
# downsample's raw output), the side output, stride, the raw map it writes
LAUNCHES = (("layer1.0.conv1", "R0", None, "X0", 1, "R1"), ("layer1.0.conv2", "R1", None, None, 1, "R2"),
            ("layer1.1.conv1", "R2", "X0", "X1", 1, "R3"), ("layer1.1.conv2", "R3", None, None, 1, "R4"),
            ("layer2.0.conv1", "R4", "X1", None, 2, "R5"), ("layer2.0.conv2", "R5", None, None, 1, "R6"),
            ("layer2.1.conv1", "R6", "Rd5", "X3", 1, "R7"), ("layer2.1.conv2", "R7", None, None, 1, "R8"),
            ("layer3.0.conv1", "R8", "X3", None, 2, "R9"), ("layer3.0.conv2", "R9", None, None, 1, "R10"),
            ("layer3.1.conv1", "R10", "Rd9", "X5", 1, "R11"), ("layer3.1.conv2", "R11", None, None, 1, "R12"))
HEAD = ("conv2", "R12", "X5")


def launch_weights(P, name, stride):
    w3, b3 = P[name]
    if stride == 2:
        w1, b1 = P[name.replace("conv1", "downsample.0")]
        return w3, b3, w1, b1
    return w3, b3, None, None


def _norm_r(R, r, st):
    """how far N(R) can move when every element of R moves by at most r: the mean by mean(r), the standard
    deviation by rms(r)"""
    if st is None:
        return r
    mean, rstd = st
    var = 1.0 / rstd ** 2 - EPS
    rho = np.sqrt((r ** 2).mean(axis=(2, 3)))
    sd = np.sqrt(np.maximum(var, 0.0))
    lo = 1.0 / np.sqrt(np.maximum(sd - rho, 0.0) ** 2 + EPS)
    hi = 1.0 / np.sqrt((sd + rho) ** 2 + EPS)
    d_rstd = np.maximum(lo - rstd, rstd - hi)[:, :, None, None]
    centred = np.abs(np.asarray(R, np.float64) - mean[:, :, None, None])
    return (r + r.mean(axis=(2, 3))[:, :, None, None]) * lo[:, :, None, None] + centred * d_rstd


def encoder(images, P, norm, round16=True):
    """The whole chain -> dict: the raw maps R0 .. R12 (Rd5, Rd9), the block outputs X0, X1, X3, X5, the staged
    operands A<k> of launch k (A5, A9 and A13 are the outputs of layer1, layer2 and layer3), the statistics S<k> =
    (mean, rstd), ``out`` (fnet) or ``net`` / ``inp`` (cnet), and r_out (r_net / r_inp)"""
    inst = norm == "instance"
    v, r = {}, {}

    def put(name, R, rr):
        c = R.shape[1] // 2
        for key, sl in ((name, slice(0, c)), ("Rd" + name[1:], slice(c, None))) if name in ("R5", "R9") else \
                ((name, slice(None)),):
            v[key], r[key] = R[:, sl], rr[:, sl]
            if inst:
                v["S" + key[1:]] = stats(v[key])[:2]

    def stored_r(val, rr):
        return rr + 0.5 * ulp_fp16(val) if round16 else rr

    R0, _ = stem(images, *P["conv1"], round16=round16)
    put("R0", R0, stored_r(R0, np.zeros_like(R0)))
    k = 1
    for name, src, second, side, stride, dst in LAUNCHES + (HEAD + (None, 1, None),):
        st = v.get("S" + src[1:])
        pst = v.get("S" + second[1:]) if second and second.startswith("Rd") else None
        a, _ = stage(v[src], st, v[second] if second else None, pst, round16)
        ra = _norm_r(v[src], r[src], st)
        if second:
            ra = ra + (_norm_r(v[second], r[second], pst) if pst is not None else r[second])
        ra = stored_r(a, ra)
        v[f"A{k}"], r[f"A{k}"] = a, ra
        if side:
            v[side], r[side] = a, ra
        if dst is None:
            break
        w3, b3, w1, b1 = launch_weights(P, name, stride)
        R, _ = conv(a, None, w3, b3, stride, w1, b1, round16)
        rr = conv2d(ra, np.abs(w3), None, stride)
        if w1 is not None:
            rr = np.concatenate([rr, conv2d(ra, np.abs(w1), None, stride)], axis=1)
        put(dst, R, stored_r(R, rr))
        k += 1
    w, b = P["conv2"]
    res, _ = head(a, None, w, b, norm, round16)
    rr = conv2d(ra, np.abs(w))
    if inst:
        v["out"], v["r_out"] = res, stored_r(res, rr)
    else:
        (v["net"], v["inp"]) = res
        v["r_net"], v["r_inp"] = stored_r(res[0], rr[:, :128]), stored_r(res[1], rr[:, 128:])
    return v


def fixture_inputs(tag):
    """Parameters and images of case ``tag`` of tests/golden/ref_basic_encoder.npz, regenerated from the frozen
    ``np.random.RandomState`` stream the generator drew them from: (norm, P, images)"""
    norm, n, H, W = FIXTURE_CASES[tag]
    rng = np.random.RandomState(FIXTURE_SEED[tag])
    P = make_params(rng, norm)
    return norm, P, make_images(rng, n, H, W)


def fixture_case(tag):
    """dict(z: the file, norm, P, images, plain / rounded: the oracle's two evaluations); computed once, never
    modified"""
    if tag not in _fixture:
        norm, P, images = fixture_inputs(tag)
        _fixture[tag] = {"z": np.load(FIXTURE, allow_pickle=False), "norm": norm, "P": P, "images": images,
                         "plain": encoder(images, P, norm, False), "rounded": encoder(images, P, norm, True)}
    return _fixture[tag]


def shape_case(norm, shape):
    """Seeded parameters, images and the oracle's two evaluations at ``shape`` = (n, H, W): dict(P, images, plain,
    rounded); computed once, never modified"""
    key = (norm, shape)
    if key not in _shape_case:
        n, H, W = shape
        rng = np.random.default_rng(100000 * n + 300 * H + W + (7 if norm == "none" else 0))
        P = make_params(rng, norm)
        images = make_images(rng, n, H, W)
        _shape_case[key] = {"P": P, "images": images, "plain": encoder(images, P, norm, False),
                            "rounded": encoder(images, P, norm, True)}
    return _shape_case[key]
