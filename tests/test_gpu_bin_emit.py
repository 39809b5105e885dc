"""The per-bin depth sort's own tile lists (k_bin_depth_sort's wave <-> tile
emit, at every bin shift) against the two other ways the library builds the
same lists: the exact per-tile pairs with no bins (WGSR_BIN_SHIFT=0) and the
Gaussian-level depth sort followed by k_expand_bins (WGSR_DEPTH_SORT=global).
The lists are the same lists, so images, radii, n_touched, num_rendered and
every gradient are compared bit for bit; one run per shape is also checked
against the CPU restatement with the tolerances of test_gpu_raster.

Shapes: the smallest at which each path of the emit can go wrong.
  64x64, one bin of 4x4 tiles, 20 000 Gaussians: a bin of more than three LDS
    tiles (kBdsCap = 5120 entries) -- the chunked emit over >= 5 chunks of
    3584, running counts carried across chunks, all 16 tiles live.
  48x40, 3x3 tiles of one 4x4 bin, 30 000 Gaussians: the same with tiles
    outside the image (waves that own an absent tile).
  100x72, 30 000 Gaussians: several bins of different lengths with partial
    bins right and bottom, at 4x4-tile bins and at 2x2-tile bins (two waves
    per tile).
  200x136, 6 000 Gaussians, default opacities: every entries-per-lane count
    from 1 up, bins of fewer than 64 entries, empty bins.
The first three set every opacity to 0.05: no pixel terminates early and
nearly every visible Gaussian reaches a list (counts of n_touched > 0 on the
CPU restatement: 17 395, 16 979, 25 914).

WGSR_BIN_DEPTH_MAX_AVG is raised for every run: bins this full would otherwise
fall back to the Gaussian-level sort, and the emit would not run at all.  Each
case asserts that the per-bin schedule really ran (it leaves no depth order:
wgsr_depth_order_offset() == -1).
"""
import numpy as np
import pytest
import torch

from test_gpu_raster import _cpu_expect, _synthetic, check_against, run_c

pytestmark = pytest.mark.gpu

K_BDS_CAP = 5120  # kBdsCap (raster_bin_sort.hip): entries k_bin_depth_sort sorts in LDS

# (W, H, P, SH degree, every opacity or None for the scene's own)
SHAPES = {
    "full_bin": (64, 64, 20_000, 0, 0.05),
    "partial_bin": (48, 40, 30_000, 0, 0.05),
    "ragged_bins": (100, 72, 30_000, 1, 0.05),
    "small_bins": (200, 136, 6_000, 1, None),
}
_cache = {}


def _inputs(shape):
    key = ("in", shape)
    if key not in _cache:
        W, H, P, deg, opac = SHAPES[shape]
        inputs, settings, grads = _synthetic(P, W, H, deg)
        if opac is not None:
            inputs = dict(inputs, opacities=torch.full_like(inputs["opacities"], opac))
        _cache[key] = (inputs, settings, grads)
    return _cache[key]


def _depth_order_offset():
    from wgsr import _lib
    return int(_lib.load().wgsr_depth_order_offset())


def _run(shape, monkeypatch, shift, sort=None):
    """One forward + backward at the given bin shift and depth schedule;
    returns (outputs, the forward's depth-order offset).  Shift 0 and the
    global schedule are computed once per (shape, shift) and shared."""
    key = ("out", shape, shift, sort)
    if sort is None or key not in _cache:
        monkeypatch.setenv("WGSR_BIN_DEPTH_MAX_AVG", "100000000")
        monkeypatch.setenv("WGSR_BIN_SHIFT", str(shift))
        if sort is None:
            monkeypatch.delenv("WGSR_DEPTH_SORT", raising=False)
        else:
            monkeypatch.setenv("WGSR_DEPTH_SORT", sort)
        offs = []
        out = run_c(*_inputs(shape), between=lambda: offs.append(_depth_order_offset()))
        if sort is None:
            return out, offs[0]
        _cache[key] = (out, offs[0])
    return _cache[key]


def _cpu(shape):
    key = ("cpu", shape)
    if key not in _cache:
        _cache[key] = _cpu_expect(*_inputs(shape))
    return _cache[key]


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k, v in a.items():
        if k == "num_rendered":
            assert b[k] == v, what
        else:
            np.testing.assert_array_equal(b[k], v, err_msg=f"{what}: {k}")


def _check(shape, shift, monkeypatch, cpu):
    out, off = _run(shape, monkeypatch, shift)
    assert off == -1, "the per-bin depth sort did not run"
    exact, _ = _run(shape, monkeypatch, 0, "bins")
    expand, off_g = _run(shape, monkeypatch, shift, "global")
    assert off_g != -1, "the Gaussian-level sort did not run"
    assert out["num_rendered"] > 0
    _same(exact, out, f"{shape} shift {shift} vs exact per-tile lists")
    _same(expand, out, f"{shape} shift {shift} vs k_expand_bins")
    if cpu:
        check_against(out, _cpu(shape))
    return out


@pytest.mark.parametrize("shape", ["full_bin", "partial_bin"])
def test_chunked_emit_of_one_big_bin(shape, monkeypatch):
    """One sort bin holds the whole frame, and more than three LDS tiles of
    entries: bds_big sorts it chunk by chunk and bds_emit_big emits the lists
    over >= 5 chunks with running per-tile counts.  Every Gaussian with
    n_touched > 0 is an entry of the bin, so their number bounds its length
    from below."""
    W, H = SHAPES[shape][:2]
    assert (W + 15) // 16 <= 4 and (H + 15) // 16 <= 4  # one 4x4-tile bin
    out = _check(shape, 2, monkeypatch, cpu=True)
    n_in_lists = int(np.count_nonzero(out["n_touched"] > 0))
    assert n_in_lists > 3 * K_BDS_CAP, n_in_lists


@pytest.mark.parametrize("shift", [2, 1])
def test_ragged_bins(shift, monkeypatch):
    """2x2 bins of 4x4 tiles (or 4x3 of 2x2) with partial bins on the right
    and bottom edges and thousands of entries each: 16 tiles over eight waves,
    and four tiles with two waves per tile."""
    _check("ragged_bins", shift, monkeypatch, cpu=shift == 2)


@pytest.mark.parametrize("shift", [2, 1])
def test_small_bins(shift, monkeypatch):
    """Default opacities on a 13x9-tile frame: short bins (every entries-per-
    lane count from 1 up, bins below one wave of entries) and empty bins."""
    _check("small_bins", shift, monkeypatch, cpu=shift == 2)
