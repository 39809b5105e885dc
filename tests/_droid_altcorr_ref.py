"""float64 numpy restatement of ``droid_backends.altcorr_forward`` /
``altcorr_backward`` (csrc/droid_altcorr.hip), and the inputs their tests share.

The op, from its definition: for pixel (y, x) of entry
b and lookup centre (x0, y0) = scale * coords[b, n, y, x], the tap at integer
position (tx, ty) is the dot product <fmap1[b, y, x, :], fmap2[b, ty, tx, :]>,
zero outside fmap2's plane; with (fx, fy) = floor(x0, y0) and (dx, dy) the
fractional parts, output (ix, iy), ix, iy in [0, 2r], stored at channel
iy + (2r+1) ix, is the bilinear blend

    (1-dx)(1-dy) tap(X, Y) + dx (1-dy) tap(X+1, Y) + (1-dx) dy tap(X, Y+1) + dx dy tap(X+1, Y+1)

with (X, Y) = (fx + ix - r, fy + iy - r).  Parity with the reference's CUDA
binary at the borders is unpinned, as for the other ops (_droid_ref.py).
"""
import functools

import numpy as np

import _droid_ref

# (B, N, H1, W1, H2, W2, C, r): odd sizes with partial tiles and H2 x W2 !=
# H1 x W1; the same at r = 1 with the smallest channel count; two tiles with
# four 32-channel passes; a plane wider and taller than the kernel's 16 x 16
# rectangle, so that a tile's taps spread over several of them
SHAPES = ((3, 2, 5, 7, 6, 9, 64, 3), (3, 2, 5, 7, 6, 9, 32, 1), (2, 1, 9, 8, 5, 16, 128, 3),
          (2, 1, 9, 10, 20, 37, 32, 3))


def _centre(coords, b, n, y, x, scale):
    x0, y0 = float(coords[b, n, y, x, 0]) * scale, float(coords[b, n, y, x, 1]) * scale
    fx, fy = np.floor(x0), np.floor(y0)
    return int(fx), int(fy), x0 - fx, y0 - fy


def _weights(dx, dy):
    # the taps (0, 0), (1, 0), (0, 1), (1, 1) as (x offset, y offset, weight)
    return ((0, 0, (1 - dx) * (1 - dy)), (1, 0, dx * (1 - dy)), (0, 1, (1 - dx) * dy), (1, 1, dx * dy))


def altcorr_forward(fmap1, fmap2, coords, r, scale=1.0):
    """(corr, mag) [B, N, (2r+1)^2, H1, W1] in float64; ``mag`` is the same
    expression on |fmap1| and |fmap2| (the blend weights are non-negative)."""
    f1, f2 = np.asarray(fmap1, np.float64), np.asarray(fmap2, np.float64)
    a1, a2 = np.abs(f1), np.abs(f2)
    B, N, H1, W1, _ = coords.shape
    H2, W2 = f2.shape[1:3]
    S, rd = 2 * r + 2, 2 * r + 1
    corr, mag = np.zeros((B, N, rd * rd, H1, W1)), np.zeros((B, N, rd * rd, H1, W1))
    for b in range(B):
        for n in range(N):
            for y in range(H1):
                for x in range(W1):
                    fx, fy, dx, dy = _centre(coords, b, n, y, x, scale)
                    taps, tmag = np.zeros((S, S)), np.zeros((S, S))  # [ky, kx]
                    for ky in range(S):
                        for kx in range(S):
                            tx, ty = fx - r + kx, fy - r + ky
                            if 0 <= tx < W2 and 0 <= ty < H2:
                                taps[ky, kx] = f1[b, y, x] @ f2[b, ty, tx]
                                tmag[ky, kx] = a1[b, y, x] @ a2[b, ty, tx]
                    for ix in range(rd):
                        for iy in range(rd):
                            for ox, oy, wgt in _weights(dx, dy):
                                corr[b, n, iy + rd * ix, y, x] += wgt * taps[iy + oy, ix + ox]
                                mag[b, n, iy + rd * ix, y, x] += wgt * tmag[iy + oy, ix + ox]
    return corr, mag


def altcorr_backward(fmap1, fmap2, coords, corr_grad, r):
    """The adjoint of the forward applied to ``corr_grad``: a dict with
    ``fmap1_grad`` / ``fmap2_grad``, their magnitudes ``mag1`` / ``mag2`` (the
    same expressions on |fmap1|, |fmap2|, |corr_grad|), ``count`` (per
    fmap2_grad element, how many (n, y, x) windows have a tap on it) and
    ``touched`` = count > 0."""
    f1, f2, cg = (np.asarray(a, np.float64) for a in (fmap1, fmap2, corr_grad))
    a1, a2, acg = np.abs(f1), np.abs(f2), np.abs(cg)
    B, N, H1, W1, _ = coords.shape
    H2, W2 = f2.shape[1:3]
    S, rd = 2 * r + 2, 2 * r + 1
    g1, g2, m1, m2 = np.zeros_like(f1), np.zeros_like(f2), np.zeros_like(f1), np.zeros_like(f2)
    count = np.zeros(f2.shape, np.int64)
    for b in range(B):
        for n in range(N):
            for y in range(H1):
                for x in range(W1):
                    fx, fy, dx, dy = _centre(coords, b, n, y, x, 1.0)
                    tg, tga = np.zeros((S, S)), np.zeros((S, S))  # d / d tap [ky, kx]
                    for ix in range(rd):
                        for iy in range(rd):
                            for ox, oy, wgt in _weights(dx, dy):
                                tg[iy + oy, ix + ox] += wgt * cg[b, n, iy + rd * ix, y, x]
                                tga[iy + oy, ix + ox] += wgt * acg[b, n, iy + rd * ix, y, x]
                    for ky in range(S):
                        for kx in range(S):
                            tx, ty = fx - r + kx, fy - r + ky
                            if 0 <= tx < W2 and 0 <= ty < H2:
                                g1[b, y, x] += tg[ky, kx] * f2[b, ty, tx]
                                m1[b, y, x] += tga[ky, kx] * a2[b, ty, tx]
                                g2[b, ty, tx] += tg[ky, kx] * f1[b, y, x]
                                m2[b, ty, tx] += tga[ky, kx] * a1[b, y, x]
                                count[b, ty, tx] += 1
    return dict(fmap1_grad=g1, fmap2_grad=g2, mag1=m1, mag2=m2, count=count, touched=count > 0)


def make_inputs(B, N, H1, W1, H2, W2, C, seed=3):
    """fmap1 [B, H1, W1, C], fmap2 [B, H2, W2, C] (float64, O(1) values; the
    caller rounds them to the type under test) and coords [B, N, H1, W1, 2]
    (float32): ``_droid_ref.make_lookup_inputs``' centres, one seed per n --
    interior points, exact integers, every border straddled, negatives,
    centres more than r + 1 outside, -40 and 1000.5.  The last entry's
    interior centres are pulled towards the origin (x 0.25) so that part of
    its fmap2 plane is under no window: fmap2_grad has untouched elements."""
    rng = np.random.default_rng(seed)
    fmap1 = rng.standard_normal((B, H1, W1, C))
    fmap2 = rng.standard_normal((B, H2, W2, C))
    coords = np.zeros((B, N, H1, W1, 2), np.float32)
    special = np.zeros(H1 * W1, bool)
    special[[(k // B) * 3 % (H1 * W1) for k in range(18) if k % B == B - 1]] = True
    for n in range(N):
        c = _droid_ref.make_lookup_inputs(B, H1, W1, H2, W2, seed=seed + 1 + n)[1]  # [B, 2, H1, W1]
        c[B - 1] = np.where(special.reshape(H1, W1), c[B - 1], np.float32(0.25) * c[B - 1])
        coords[:, n] = np.moveaxis(c, 1, -1)
    return fmap1, fmap2, coords


def forward_bound(mag, C, ref=None, half=False):
    """|got - ref| allowed: gamma_n for C products summed in any order plus the
    weight and blend roundings; for float16 output one more rounding of the
    result."""
    bound = 1.01 * (C + 16) * 2.0 ** -24 * mag
    if half:
        bound = bound + 2.0 ** -10 * np.abs(ref) + 2.0 ** -24
    return bound


@functools.lru_cache(maxsize=None)
def forward_case(index, half=False):
    """The inputs of SHAPES[index], rounded to float32 or float16, with the
    oracle's (corr, mag) on the rounded values.  Shared: do not modify."""
    B, N, H1, W1, H2, W2, C, r = SHAPES[index]
    fmap1, fmap2, coords = make_inputs(B, N, H1, W1, H2, W2, C)
    dt = np.float16 if half else np.float32
    fmap1, fmap2 = fmap1.astype(dt), fmap2.astype(dt)
    corr, mag = altcorr_forward(fmap1, fmap2, coords, r)
    return dict(fmap1=fmap1, fmap2=fmap2, coords=coords, r=r, C=C, corr=corr, mag=mag)


@functools.lru_cache(maxsize=None)
def backward_case(index):
    """float32 inputs of SHAPES[index], an upstream gradient, and the oracle's
    backward.  Shared: do not modify."""
    case = forward_case(index)
    r = case["r"]
    shape = case["coords"].shape[:2] + ((2 * r + 1) ** 2,) + case["coords"].shape[2:4]
    corr_grad = np.random.default_rng(11 + index).standard_normal(shape).astype(np.float32)
    ref = altcorr_backward(case["fmap1"], case["fmap2"], case["coords"], corr_grad, r)
    return dict(case, corr_grad=corr_grad, **ref)
