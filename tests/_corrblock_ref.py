"""float64 numpy oracle of the all-pairs correlation pyramid (corr.py CorrBlock
as it runs under autocast; csrc/droid_corrvol.hip, wgsr.frontend.CorrBlock).

Level 0 of an edge is round_fp16 of the dot product over the channels of
fmap1[:, p1] / 4 and fmap2[:, p2] / 4 -- here the exact dot product of the fp16
inputs over 16 (float64 holds it: 22-bit products, at most a few hundred of
them).  Level i + 1 is round_fp16 of the mean of the 2 x 2 block of level i's
ROUNDED values, an odd trailing row or column dropped (avg_pool2d).  The lookup
is tests/_droid_ref.corr_index_forward per level at coords / 2^i, the windows
concatenated along the channels.  Nothing here imports the package under test.
"""
import numpy as np

import _droid_ref as R


def round_fp16(x):
    """The float16 nearest to each float64 value (ties to even), as float64."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def ulp16(x):
    """The spacing of float16 at magnitude |x| (2^-24 below the normal range)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def make_maps(e, c, h, w, seed, h2=None, w2=None):
    """fmap1 [e, c, h, w], fmap2 [e, c, h2, w2]: standard normal, rounded to float16."""
    rng = np.random.default_rng(seed)
    h2, w2 = h2 or h, w2 or w
    return (rng.standard_normal((e, c, h, w)).astype(np.float16),
            rng.standard_normal((e, c, h2, w2)).astype(np.float16))


def level0_exact(fmap1, fmap2):
    """(exact, mag) [e, h1, w1, h2, w2]: the dot product of the fp16 inputs over
    16, and the same dot product of their absolute values."""
    e, c, h1, w1 = fmap1.shape
    _, _, h2, w2 = fmap2.shape
    a = fmap1.astype(np.float64).reshape(e, c, h1 * w1)
    b = fmap2.astype(np.float64).reshape(e, c, h2 * w2)
    exact = np.matmul(a.transpose(0, 2, 1), b) / 16.0
    mag = np.matmul(np.abs(a).transpose(0, 2, 1), np.abs(b)) / 16.0
    return exact.reshape(e, h1, w1, h2, w2), mag.reshape(e, h1, w1, h2, w2)


def level0_bound(got, exact, mag, c):
    """One fp16 rounding plus any-order fp32 accumulation of c products."""
    return 0.5 * ulp16(np.maximum(np.abs(got), np.abs(exact))) + (c + 1) * 2.0 ** -24 * mag


def pool(level):
    """round_fp16 of the 2 x 2 mean over the last two dimensions."""
    level = np.asarray(level, np.float64)
    h, w = level.shape[-2] // 2, level.shape[-1] // 2
    v = level[..., :2 * h, :2 * w]
    s = (v[..., 0::2, 0::2] + v[..., 0::2, 1::2]) + (v[..., 1::2, 0::2] + v[..., 1::2, 1::2])
    return round_fp16(s / 4.0)  # (four fp16 values: the float64 sum is exact)


def pyramid(fmap1, fmap2, num_levels=4):
    """The levels [e, h1, w1, h2 >> i, w2 >> i] (float64 holding fp16 values)."""
    exact, _ = level0_exact(fmap1, fmap2)
    levels = [round_fp16(exact)]
    for _ in range(num_levels - 1):
        levels.append(pool(levels[-1]))
    return levels


def lookup(levels, coords, r):
    """[e, L (2r+1)^2, h, w] float64 of coords [e, h, w, 2] (x, y; float32):
    level i's window, first index along x, in channels [i (2r+1)^2, (i+1) (2r+1)^2)."""
    coords = np.ascontiguousarray(np.asarray(coords, np.float32).transpose(0, 3, 1, 2))
    e, _, h, w = coords.shape
    out = []
    for i, level in enumerate(levels):
        c = (coords / np.float32(2 ** i)).astype(np.float32)
        out.append(R.corr_index_forward(level, c, r).reshape(e, -1, h, w))
    return np.concatenate(out, axis=1)


def make_coords(e, h, w, seed=1):
    """coords [e, h, w, 2] float32 in _droid_ref.make_lookup_inputs' style: interior
    points, exact integers, every border straddled, negative values and centres
    beyond r + 1 outside the plane (the plane is level 0's, h x w)."""
    _, c = R.make_lookup_inputs(e, h, w, h, w, seed)
    return np.ascontiguousarray(c.transpose(0, 2, 3, 1))
