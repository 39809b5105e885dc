"""GPU tests of the fused correlation pyramid (csrc/droid_corrvol.hip:
k_corrvol_build, k_corrvol_lookup; wgsr.frontend.CorrBlock) against the float64
oracle of tests/_corrblock_ref.py.

Cases (E, C, H x W): 3 x 32 x 9 x 11 (odd in both: partial tiles of frame-1
pixels and of frame-2 bands, level 3 is 1 x 1, a trailing row and column
dropped at every level, element moves); 2 x 96 x 8 x 8 (exactly one patch, C
no power of two); 2 x 128 x 12 x 16 (a full and a half band, 16-byte moves);
1 x 128 x 48 x 64 (the tracker's shape: full-width bands, a 19 MB level 0).
The maps are standard normal rounded to fp16; the edges go to a non-identity
permutation of slots inside a larger store whose every element was set to a
constant beforehand.

Tolerances.  Level 0: |got - exact| <= 1/2 ulp16 + (C + 1) 2^-24 sum|a||b|
per element -- one fp16 rounding and any-order fp32 accumulation of C products
(ulp16 at the larger of |got| and |exact|; sum|a||b| the same dot product on
absolute values); nothing fitted.  A pooled level, against round_fp16 of the
float64 mean of the 2 x 2 block the kernel itself stored one level down: at
least 99 % exactly equal and the rest within one ulp16 (a block whose four
values span so many binades that their fp32 sum is inexact).  Lookup against
the oracle on the kernel's own levels: the fp16 lookup tolerance of
tests/test_gpu_droid.py, |d| <= 2^-10 |ref| + 1e-6 max|input|.  Against
droid_backends.corr_index_forward per level, and between blocks that hold the
same edges: bit-identical.
"""
import functools

import numpy as np
import pytest
import torch

import _corrblock_ref as CR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LEVELS, RADIUS = 4, 3
POISON = 1234.0
CASES = {"3x32x9x11": (3, 32, 9, 11), "2x96x8x8": (2, 96, 8, 8), "2x128x12x16": (2, 128, 12, 16),
         "1x128x48x64": (1, 128, 48, 64)}
# edge k -> slot, in a store of E + 3 slots
SLOTS = {3: [4, 0, 2], 2: [3, 1], 1: [2]}


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def maps(name):
    e, c, h, w = CASES[name]
    return CR.make_maps(e, c, h, w, seed=5)


@functools.lru_cache(maxsize=None)
def built(name):
    """The case's edges built once into permuted slots of a poisoned store:
    (store, slots tensor, offsets, slot_elems, levels as float64 numpy in edge order)."""
    from wgsr import frontend
    e, c, h, w = CASES[name]
    fmap1, fmap2 = maps(name)
    offsets, elems = frontend.corr_slot_layout(h, w, LEVELS)
    store = torch.full(((e + 3) * elems,), POISON, dtype=torch.float16, device=DEV)
    slots = dev(np.array(SLOTS[e], np.int32))
    frontend.corr_build(dev(fmap1), dev(fmap2), store, slots, LEVELS)
    torch.cuda.synchronize()
    rows = store.view(e + 3, elems)[slots.long()].cpu().numpy()
    levels = [rows[:, off:off + h * w * (h >> i) * (w >> i)].reshape(e, h, w, h >> i, w >> i).astype(np.float64)
              for i, off in enumerate(offsets)]
    return store, slots, offsets, elems, levels


@pytest.mark.parametrize("name", CASES)
def test_level0_is_the_rounded_dot_product(name):
    e, c, h, w = CASES[name]
    got = built(name)[4][0]
    exact, mag = CR.level0_exact(*maps(name))
    ratio = np.abs(got - exact) / CR.level0_bound(got, exact, mag, c)
    print("level 0: worst |d| / bound", ratio.max(), "exactly the oracle's rounding",
          (got == CR.round_fp16(exact)).mean())
    assert np.isfinite(got).all() and ratio.max() <= 1.0


@pytest.mark.parametrize("name", CASES)
def test_pooled_levels_average_what_was_stored(name):
    levels = built(name)[4]
    for i in range(1, LEVELS):
        ref = CR.pool(levels[i - 1])
        assert levels[i].shape == ref.shape
        same = levels[i] == ref
        off = np.abs(levels[i] - ref) / CR.ulp16(np.maximum(np.abs(levels[i]), np.abs(ref)))
        print(f"level {i}: exactly equal {same.mean():.4%}, worst distance {off.max()} ulp16")
        assert same.mean() >= 0.99 and off.max() <= 1.0
    # the check tells the two apart: pooling the unrounded level 0 would miss it
    exact, _ = CR.level0_exact(*maps(name))
    assert (CR.pool(exact) == levels[1]).mean() < 0.99


@pytest.mark.parametrize("name", CASES)
def test_unused_slots_and_padding_keep_their_poison(name):
    e, c, h, w = CASES[name]
    store, slots, offsets, elems, _ = built(name)
    rows = store.view(e + 3, elems)
    unused = sorted(set(range(e + 3)) - set(SLOTS[e]))
    assert len(unused) == 3 and bool((rows[unused] == POISON).all())
    # the alignment padding between the levels of a used slot
    for i, off in enumerate(offsets):
        end = off + h * w * (h >> i) * (w >> i)
        nxt = offsets[i + 1] if i + 1 < LEVELS else elems
        assert bool((rows[SLOTS[e]][:, end:nxt] == POISON).all())


def lookup_close(got, ref, scale):
    d = np.abs(got.astype(np.float64) - ref)
    bound = 2.0 ** -10 * np.abs(ref) + 1e-6 * scale
    print("worst |d| / bound", (d / bound).max())
    return bool((d <= bound).all())


@pytest.mark.parametrize("name,r", [(n, RADIUS) for n in CASES] + [("3x32x9x11", 1)])
def test_lookup_matches_the_oracle_on_the_kernels_own_levels(name, r):
    from wgsr import frontend
    e, c, h, w = CASES[name]
    store, slots, _, _, levels = built(name)
    coords = CR.make_coords(e, h, w)
    got = frontend.corr_lookup(store, slots, dev(coords), LEVELS, r)
    assert got.shape == (e, LEVELS * (2 * r + 1) ** 2, h, w) and got.dtype == torch.float16
    ref = CR.lookup(levels, coords, r)
    assert lookup_close(got.float().cpu().numpy(), ref, max(np.abs(level).max() for level in levels))


def block_of(name, capacity=None):
    from wgsr.frontend import CorrBlock
    fmap1, fmap2 = maps(name)
    return CorrBlock(dev(fmap1)[None], dev(fmap2)[None], num_levels=LEVELS, radius=RADIUS, capacity=capacity)


def reference_lookup(pyramid, coords, r):
    """The reference's CorrBlock.__call__ (corr.py:57-67) over this project's op."""
    import droid_backends
    batch, num, ht, wd, _ = coords.shape
    c = coords.permute(0, 1, 4, 2, 3).contiguous().view(batch * num, 2, ht, wd)
    out = [droid_backends.corr_index_forward(level, c / 2 ** i, r)[0].view(batch, num, -1, ht, wd)
           for i, level in enumerate(pyramid)]
    return torch.cat(out, dim=2)


@pytest.mark.parametrize("name", CASES)
def test_lookup_is_bit_identical_to_the_per_level_op(name):
    e, c, h, w = CASES[name]
    block = block_of(name, capacity=e + 2)
    pyramid = block.corr_pyramid
    assert [tuple(p.shape) for p in pyramid] == [(e, h, w, h >> i, w >> i) for i in range(LEVELS)]
    # the block's levels are the directly built ones
    for p, level in zip(pyramid, built(name)[4]):
        assert np.array_equal(p.cpu().numpy().astype(np.float64), level)
    coords = dev(CR.make_coords(e, h, w))[None]
    got = block(coords)
    assert got.shape == (1, e, LEVELS * 49, h, w) and got.dtype == torch.float16
    assert torch.equal(got, reference_lookup(pyramid, coords, RADIUS))


# ---------------------------------------------------------------------------
# append, cat, block[index]
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seven():
    f1, f2 = CR.make_maps(7, 32, 9, 11, seed=9)
    return dev(f1)[None], dev(f2)[None], dev(CR.make_coords(7, 9, 11, seed=2))[None]


def same_as_built_in_one_go(block, edges):
    from wgsr.frontend import CorrBlock
    f1, f2, coords = seven()
    idx = torch.tensor(edges, device=DEV)
    ref = CorrBlock(f1[:, idx], f2[:, idx], num_levels=LEVELS, radius=RADIUS)
    assert len(block) == len(edges)
    for a, b in zip(block.corr_pyramid, ref.corr_pyramid):
        assert torch.equal(a, b)
    assert torch.equal(block(coords[:, idx].contiguous()), ref(coords[:, idx].contiguous()))


def test_append_cat_and_mask_equal_a_block_built_in_one_go():
    from wgsr.frontend import CorrBlock
    f1, f2, _ = seven()
    block = CorrBlock(f1[:, :3], f2[:, :3], num_levels=LEVELS, radius=RADIUS)
    assert block.capacity == 3
    assert block.append(f1[:, 3:5], f2[:, 3:5]) is block  # full: the store doubles
    assert block.capacity == 6
    same_as_built_in_one_go(block, [0, 1, 2, 3, 4])
    mask = torch.tensor([True, False, True, True, False], device=DEV)
    assert block[mask] is block
    same_as_built_in_one_go(block, [0, 2, 3])
    before = block._store.data_ptr()
    block.append(f1[:, 5:7], f2[:, 5:7])  # into the freed slots
    assert block._table.slots == [0, 2, 3, 1, 4] and block.capacity == 6 and block._store.data_ptr() == before
    same_as_built_in_one_go(block, [0, 2, 3, 5, 6])
    # cat: the other block's edges, copied; with a growth of the store (5 + 3 > 6)
    other = CorrBlock(f1[:, 4:7], f2[:, 4:7], num_levels=LEVELS, radius=RADIUS, capacity=4)
    assert block.cat(other) is block and block.capacity == 12
    same_as_built_in_one_go(block, [0, 2, 3, 5, 6, 4, 5, 6])
    # an integer index and a slice, as they index a tensor's first dimension
    block[torch.tensor([7, 0, 5], device=DEV)]
    same_as_built_in_one_go(block, [6, 0, 4])
    block[1:]
    same_as_built_in_one_go(block, [0, 4])
    same_as_built_in_one_go(other, [4, 5, 6])  # (untouched by cat)


def test_calls_allocate_no_more_than_they_must():
    from wgsr import frontend
    from wgsr.frontend import CorrBlock
    f1, f2 = (dev(a)[None] for a in CR.make_maps(6, 128, 12, 16, seed=4))
    coords = dev(CR.make_coords(6, 12, 16))[None]
    slot_bytes = 2 * frontend.corr_slot_layout(12, 16, LEVELS)[1]
    block = CorrBlock(f1[:, :4], f2[:, :4], num_levels=LEVELS, radius=RADIUS, capacity=8)
    new1, new2 = f1[:, 4:].contiguous(), f2[:, 4:].contiguous()
    mask = torch.tensor([True, False, True, True], device=DEV)
    block(coords[:, :4].contiguous())
    torch.cuda.synchronize()

    def growth(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    grew, _ = growth(lambda: block[mask])
    print("block[mask] peak growth", grew, "one slot", slot_bytes)
    assert grew < slot_bytes and len(block) == 3
    grew, _ = growth(lambda: block.append(new1, new2))
    print("append peak growth", grew, "one slot", slot_bytes)
    assert grew < slot_bytes and len(block) == 5 and block.capacity == 8
    c5 = coords[:, :5].contiguous()
    block(c5)  # (the device copy of the slot table is made)
    grew, out = growth(lambda: block(c5))
    out_bytes = out.numel() * 2
    print("lookup peak growth", grew, "output", out_bytes)
    assert out_bytes <= grew <= (out_bytes + 511) // 512 * 512


def test_refusals():
    from wgsr import frontend
    from wgsr.frontend import CorrBlock
    f1, f2, coords = seven()
    with pytest.raises(NotImplementedError, match="float32"):
        CorrBlock(f1.float(), f2.float())
    with pytest.raises(RuntimeError, match="at least 8"):
        CorrBlock(f1[..., :7, :].contiguous(), f2[..., :7, :].contiguous())
    with pytest.raises(RuntimeError, match="at least 8"):
        CorrBlock(f1[..., :6].contiguous(), f2[..., :6].contiguous())
    with pytest.raises(NotImplementedError, match="requires grad"):
        CorrBlock(f1.clone().requires_grad_(True), f2)
    with torch.no_grad():  # (grad mode off: the same maps are taken)
        assert len(CorrBlock(f1[:, :1].clone().requires_grad_(True), f2[:, :1])) == 1
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        CorrBlock(f1.cpu(), f2.cpu())
    block = CorrBlock(f1[:, :2], f2[:, :2])
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        block(coords[:, :2].cpu())
    with pytest.raises(RuntimeError, match="coords must be"):
        block(coords[:, :3].contiguous())              # three edges' coords for two edges
    with pytest.raises(RuntimeError, match="coords must be"):
        block(coords[:, :2, :8].contiguous())           # another height
    with pytest.raises(RuntimeError, match="coords must be"):
        block(coords[:, :2].permute(0, 1, 4, 2, 3).contiguous())  # the sampler's layout
    with pytest.raises(RuntimeError, match="coords must be"):
        block(coords[:, :2].double())
    with pytest.raises(RuntimeError, match="like the block's"):
        block.append(f1[:, :1, :, :8].contiguous(), f2[:, :1, :, :8].contiguous())
    with pytest.raises(NotImplementedError, match="float32"):
        frontend.corr_build(f1[0].float(), f2[0].float(), block._store, block._slots(), LEVELS)


def test_build_and_lookup_capture_into_a_graph():
    """Neither launch reads anything on the host: one build plus one lookup are
    captured, and the replay gives the eager result bit for bit."""
    from wgsr import frontend
    name = "2x128x12x16"
    e, c, h, w = CASES[name]
    store0, slots, _, elems, _ = built(name)
    fmap1, fmap2 = (dev(a) for a in maps(name))
    coords = dev(CR.make_coords(e, h, w))
    out0 = frontend.corr_lookup(store0, slots, coords, LEVELS, RADIUS)
    store1 = torch.full_like(store0, POISON)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frontend.corr_build(fmap1, fmap2, store1, slots, LEVELS)
        out1 = frontend.corr_lookup(store1, slots, coords, LEVELS, RADIUS)
    store1.fill_(POISON)
    out1.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(store0, store1) and torch.equal(out0, out1)
