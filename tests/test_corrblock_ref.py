"""CPU tests of the correlation-pyramid oracle (tests/_corrblock_ref.py) and of
the slot bookkeeping of ``wgsr.frontend.CorrBlock`` (no GPU needed).

(a) The oracle against the reference's three torch calls run on the CPU in
    float16 (``matmul`` of the maps / 4, then ``avg_pool2d``).  Level 0: for
    every element |torch - exact| <= 1/2 ulp16 + (C + 1) 2^-24 sum|a||b| (one
    fp16 rounding, any-order fp32 accumulation; ulp16 at the larger of the two
    magnitudes).  Pooled levels: torch's equal the oracle's pooling of torch's
    own previous level exactly.
(b) The oracle against tests/golden/ref_corrblock.npz, recorded from the
    reference's own ``CorrBlock.__init__`` (tests/golden/make_corrblock_fixtures.py):
    which map leads, the 1 / 16 scale, the pooling floor.
(c) ``SlotTable``: take, release, grow by doubling; boolean-mask, integer-tensor
    and slice indexing; edge order kept, freed slots reused.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _corrblock_ref as CR
from _util import GOLDEN

# (E, C, H1, W1, H2, W2)
CASES = [(2, 128, 8, 8, 8, 8), (3, 32, 9, 11, 17, 25), (1, 128, 12, 16, 12, 16)]


def torch_chain(fmap1, fmap2, num_levels):
    """The reference's composition (corr.py:46-55, 85-88) on the CPU in float16."""
    e, c, h1, w1 = fmap1.shape
    _, _, h2, w2 = fmap2.shape
    a = torch.from_numpy(fmap1).reshape(e, c, h1 * w1) / 4.0
    b = torch.from_numpy(fmap2).reshape(e, c, h2 * w2) / 4.0
    corr = torch.matmul(a.transpose(1, 2), b).reshape(e * h1 * w1, 1, h2, w2)
    levels = []
    for i in range(num_levels):
        assert corr.dtype == torch.float16
        levels.append(corr.view(e, h1, w1, h2 >> i, w2 >> i).numpy().astype(np.float64))
        if i + 1 < num_levels:  # (the reference pools once more and drops the result)
            corr = F.avg_pool2d(corr, kernel_size=2, stride=2)
    return levels


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_oracle_matches_the_torch_composition(case):
    e, c, h1, w1, h2, w2 = case
    fmap1, fmap2 = CR.make_maps(e, c, h1, w1, seed=3, h2=h2, w2=w2)
    exact, mag = CR.level0_exact(fmap1, fmap2)
    got = torch_chain(fmap1, fmap2, 4)
    ratio = np.abs(got[0] - exact) / CR.level0_bound(got[0], exact, mag, c)
    print("level 0: worst |d| / bound", ratio.max())
    assert ratio.max() <= 1.0
    for i in range(1, 4):
        assert got[i].shape == (e, h1, w1, h2 >> i, w2 >> i)
        same = got[i] == CR.pool(got[i - 1])
        print(f"level {i}: exactly equal {same.mean():.4%}")
        assert same.all()


def test_oracle_matches_the_recorded_reference():
    z = np.load(os.path.join(GOLDEN, "ref_corrblock.npz"))
    fmap1, fmap2 = z["fmap1"], z["fmap2"]
    assert fmap1.dtype == np.float16 and fmap1.shape == (2, 32, 9, 11)
    exact, mag = CR.level0_exact(fmap1, fmap2)
    l0 = z["level0"].astype(np.float64)
    assert l0.shape == (2, 9, 11, 9, 11)
    ratio = np.abs(l0 - exact) / CR.level0_bound(l0, exact, mag, 32)
    print("level 0: worst |d| / bound", ratio.max())
    assert ratio.max() <= 1.0
    # the leading pixel pair is fmap1's: the transposed product would sit here
    swapped = exact.transpose(0, 3, 4, 1, 2)
    assert np.abs(l0 - swapped).max() > 0.5
    # the oracle's own pyramid agrees wherever its level 0 rounds as the reference's did
    levels = CR.pyramid(fmap1, fmap2, 3)
    print("level 0 equal to the oracle's rounding", (levels[0] == l0).mean())
    assert (levels[0] == l0).mean() >= 0.99
    prev = l0
    assert sorted(z.files) == ["fmap1", "fmap2", "level0", "level1", "level2"]  # (recorded with 3 levels)
    for i, shape in ((1, (4, 5)), (2, (2, 2))):
        got = z[f"level{i}"].astype(np.float64)
        assert got.shape == (2, 9, 11) + shape
        assert np.array_equal(got, CR.pool(prev))
        prev = got


def test_lookup_oracle_concatenates_the_levels_along_x_first():
    """One level-0 plane with a single 1 at (y, x) = (2, 5): a centre there puts it at
    window index i = r along x, j = r along y; at level 1 the pooled 0.25 at (1, 2)."""
    r = 1
    level0 = np.zeros((1, 8, 8, 8, 8))
    level0[0, :, :, 2, 5] = 1.0
    levels = [level0, CR.pool(level0)]
    coords = np.zeros((1, 8, 8, 2), np.float32)
    coords[..., 0], coords[..., 1] = 4.0, 2.0  # one to the left of the 1
    out = CR.lookup(levels, coords, r)
    assert out.shape == (1, 2 * 9, 8, 8)
    win0 = out[0, :9, 3, 3].reshape(3, 3)  # [i along x, j along y]
    assert win0[2, 1] == 1.0 and win0.sum() == 1.0
    win1 = out[0, 9:, 3, 3].reshape(3, 3)  # centre (2, 1) at level 1: the 0.25 sits on it
    assert win1[1, 1] == 0.25 and win1.sum() == 0.25


# ---------------------------------------------------------------------------
# (c) the slot table
# ---------------------------------------------------------------------------
def test_slot_table_take_release_and_grow():
    from wgsr.frontend import SlotTable
    t = SlotTable(4)
    assert t.take(3) == [0, 1, 2] and t.capacity == 4 and t.free == 1 and len(t) == 3
    assert t.take(3) == [3, 4, 5]          # full: doubled once
    assert t.capacity == 8 and t.free == 2 and t.slots == [0, 1, 2, 3, 4, 5]
    assert t.take(11)[:2] == [6, 7]        # doubled twice (8 -> 16 -> 32)
    assert t.capacity == 32 and len(t) == 17 and t.free == 15
    assert sorted(t.slots) == list(range(17))
    with pytest.raises(ValueError):
        SlotTable(0)


def test_slot_table_indexing_keeps_order_and_reuses_freed_slots():
    from wgsr.frontend import SlotTable
    t = SlotTable(8)
    t.take(6)
    mask = torch.tensor([True, False, True, True, False, True])
    assert t.select(mask) == [0, 2, 3, 5] and t.slots == [0, 2, 3, 5] and t.capacity == 8 and t.free == 4
    assert t.take(3) == [1, 4, 6]          # the freed slots first, lowest first
    assert t.slots == [0, 2, 3, 5, 1, 4, 6]
    assert t.select(torch.tensor([6, 0, 3])) == [6, 0, 5]   # an integer tensor: its order
    assert t.free == 5
    assert t.take(1) == [1]
    assert t.select(slice(1, None)) == [0, 5, 1] and t.free == 5
    assert t.select(torch.tensor([0, 0, 2])) == [0, 0, 1]   # an edge twice: one slot, held
    assert t.free == 6
    assert t.select(torch.zeros(3, dtype=torch.bool)) == [] and t.free == 8 and len(t) == 0
    assert t.take(2) == [0, 1]


def test_slot_layout_matches_the_library():
    from wgsr import _lib, frontend
    L = _lib.load()
    for h, w, levels in ((48, 64, 4), (9, 11, 4), (8, 8, 4), (12, 16, 3), (5, 7, 1)):
        offsets, elems = frontend.corr_slot_layout(h, w, levels)
        assert L.wgsr_droid_corr_slot_bytes(h, w, levels) == 2 * elems
        assert all(o % 8 == 0 for o in offsets) and elems % 8 == 0
        sizes = [h * w * (h >> i) * (w >> i) for i in range(levels)]
        assert all(offsets[i] + sizes[i] <= (offsets[i + 1] if i + 1 < levels else elems) for i in range(levels))
    # one edge at the tracker's operating point: 3072^2 (1 + 1/4 + 1/16 + 1/64) fp16
    assert frontend.corr_slot_layout(48, 64, 4)[1] * 2 == 25067520
    assert L.wgsr_droid_corr_slot_bytes(4, 64, 4) == -1   # too small for 4 levels
    assert b"at least 8" in L.wgsr_last_error()


def test_entry_points_refuse_float32_by_name_before_any_launch():
    from wgsr import _lib
    L = _lib.load()
    assert L.wgsr_droid_corr_build(None, None, 0, 1, 32, 8, 8, 4, None, 1, None, None) != 0
    assert b"WGSR_DTYPE_F32" in L.wgsr_last_error()
    assert L.wgsr_droid_corr_lookup(None, 1, None, None, 0, 1, 8, 8, 4, 3, None, None) != 0
    assert b"WGSR_DTYPE_F32" in L.wgsr_last_error()
    assert L.wgsr_droid_corr_build(None, None, 1, 1, 24, 8, 8, 4, None, 1, None, None) != 0
    assert b"multiple of 32" in L.wgsr_last_error()
    assert L.wgsr_droid_corr_lookup(None, 1, None, None, 1, 1, 8, 8, 4, 7, None, None) != 0
    assert b"radius" in L.wgsr_last_error()
    assert L.wgsr_droid_corr_build(None, None, 1, 1, 32, 8, 8, 4, None, 1, None, None) != 0
    assert b"null pointer" in L.wgsr_last_error()


def test_corrblock_validates_on_the_host():
    from wgsr.frontend import CorrBlock
    f = torch.zeros(1, 2, 32, 8, 8, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="float32"):
        CorrBlock(f.float(), f.float())
    with pytest.raises(RuntimeError, match="at least 8"):
        CorrBlock(f[..., :4, :], f[..., :4, :])
    with pytest.raises(NotImplementedError, match="requires grad"):
        CorrBlock(f.clone().requires_grad_(True), f)
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        CorrBlock(f, f)
