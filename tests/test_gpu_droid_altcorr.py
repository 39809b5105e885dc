"""GPU tests of ``droid_backends.altcorr_forward`` / ``altcorr_backward``
(csrc/droid_altcorr.hip) and ``wgsr.frontend.AltCorrBlock`` against the float64
oracle of tests/_droid_altcorr_ref.py.

Tolerances, with ``mag`` the oracle's expression on the inputs' magnitudes.
Forward: |got - ref| <= 1.01 (C + 16) 2^-24 mag -- the gamma_n bound of C
products summed in any order, plus the weight and blend roundings; an fp16
output adds 2^-10 |ref| + 2^-24 for its one rounding (the oracle reads the
fp16-rounded inputs); where mag is 0 the output is exactly 0.  Two GPU
evaluations agree within twice the bound.  Backward: fmap1_grad within 1.01
(N (2r+2)^2 + 16) 2^-24 mag1 (that many terms per element), fmap2_grad within
1.01 (count + 16) 2^-24 mag2 with ``count`` the element's number of
contributions, and exactly 0 where nothing contributes.
"""
import numpy as np
import pytest
import torch

import _droid_altcorr_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = range(len(A.SHAPES))


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def check(name, got, ref, bound):
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    live = bound > 0
    print(name, "worst error / bound", float((err[live] / bound[live]).max()) if live.any() else 0.0,
          "worst error", float(err.max()))
    assert np.isfinite(got).all()
    assert (err <= bound).all()


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("index", CASES)
def test_forward_matches_the_oracle(index, half):
    import droid_backends
    case = A.forward_case(index, half)
    out = droid_backends.altcorr_forward(dev(case["fmap1"]), dev(case["fmap2"]), dev(case["coords"]), case["r"])
    assert isinstance(out, list) and len(out) == 1
    corr = out[0]
    assert corr.dtype == (torch.float16 if half else torch.float32)
    assert tuple(corr.shape) == case["corr"].shape and corr.is_contiguous()
    got = corr.float().cpu().numpy()
    check("forward", got, case["corr"], A.forward_bound(case["mag"], case["C"], case["corr"], half))
    assert (got[case["mag"] == 0] == 0).all()


@pytest.mark.parametrize("index", CASES)
def test_forward_agrees_with_the_lookup_of_the_matmul_volume(index):
    import droid_backends
    case = A.forward_case(index)
    f1, f2, coords = dev(case["fmap1"]), dev(case["fmap2"]), dev(case["coords"])
    B, N, H1, W1 = coords.shape[:4]
    H2, W2, C = f2.shape[1:]
    corr, = droid_backends.altcorr_forward(f1, f2, coords, case["r"])
    volume = torch.matmul(f1.view(B, H1 * W1, C), f2.view(B, H2 * W2, C).transpose(1, 2)).view(B, H1, W1, H2, W2)
    bound = 2 * A.forward_bound(case["mag"], case["C"])
    for n in range(N):
        ref, = droid_backends.corr_index_forward(volume, coords[:, n].permute(0, 3, 1, 2).contiguous(), case["r"])
        check("composition", corr[:, n].cpu().numpy(), ref.view(B, -1, H1, W1).double().cpu().numpy(), bound[:, n])


def test_forward_from_a_two_byte_aligned_map():
    """A contiguous view one element into a flat buffer: the base is not
    16-byte aligned, so the kernel must load element by element."""
    import droid_backends
    case = A.forward_case(0, True)
    maps = []
    for a in (case["fmap1"], case["fmap2"]):
        flat = torch.zeros(a.size + 8, dtype=torch.float16, device=DEV)
        flat[1:1 + a.size] = dev(a).reshape(-1)
        view = flat[1:1 + a.size].view(a.shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 2
        maps.append(view)
    corr, = droid_backends.altcorr_forward(maps[0], maps[1], dev(case["coords"]), case["r"])
    check("unaligned", corr.float().cpu().numpy(), case["corr"],
          A.forward_bound(case["mag"], case["C"], case["corr"], True))


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
def check_backward(case, g1, g2, gc):
    B, N, H1, W1 = case["coords"].shape[:4]
    S = 2 * case["r"] + 2
    assert g1.dtype == g2.dtype == gc.dtype == torch.float32
    assert tuple(g1.shape) == case["fmap1"].shape and tuple(g2.shape) == case["fmap2"].shape
    assert tuple(gc.shape) == (B, N, H1, W1, 2) and not gc.any()
    check("fmap1_grad", g1.cpu().numpy(), case["fmap1_grad"], 1.01 * (N * S * S + 16) * 2.0 ** -24 * case["mag1"])
    got2 = g2.cpu().numpy()
    check("fmap2_grad", got2, case["fmap2_grad"], 1.01 * (case["count"] + 16) * 2.0 ** -24 * case["mag2"])
    assert (got2[~case["touched"]] == 0).all()


@pytest.mark.parametrize("index", CASES)
def test_backward_matches_the_oracle(index):
    import droid_backends
    case = A.backward_case(index)
    out = droid_backends.altcorr_backward(dev(case["fmap1"]), dev(case["fmap2"]), dev(case["coords"]),
                                          dev(case["corr_grad"]), case["r"])
    assert isinstance(out, list) and len(out) == 3
    check_backward(case, *out)


class CorrLayer(torch.autograd.Function):
    """The shape of the reference's autograd wrapper of the pair."""

    @staticmethod
    def forward(ctx, fmap1, fmap2, coords, r):
        import droid_backends
        ctx.r = r
        ctx.save_for_backward(fmap1, fmap2, coords)
        corr, = droid_backends.altcorr_forward(fmap1, fmap2, coords, r)
        return corr

    @staticmethod
    def backward(ctx, grad_corr):
        import droid_backends
        fmap1, fmap2, coords = ctx.saved_tensors
        g1, g2, gc = droid_backends.altcorr_backward(fmap1, fmap2, coords, grad_corr.contiguous(), ctx.r)
        return g1, g2, gc, None


def test_autograd_function_with_a_non_contiguous_gradient():
    case = A.backward_case(0)
    f1, f2 = dev(case["fmap1"]).requires_grad_(), dev(case["fmap2"]).requires_grad_()
    coords = dev(case["coords"]).requires_grad_()
    corr = CorrLayer.apply(f1, f2, coords, case["r"])
    upstream = dev(case["corr_grad"]).transpose(3, 4).contiguous().transpose(3, 4)
    assert not upstream.is_contiguous()
    corr.backward(upstream)
    check_backward(case, f1.grad, f2.grad, coords.grad)


# ---------------------------------------------------------------------------
# frontend.AltCorrBlock
# ---------------------------------------------------------------------------
LEVELS, RADIUS = 4, 3
II, JJ = (0, 0, 1, 2, 3, 4), (1, 2, 1, 3, 4, 0)  # a repeated frame, and one edge from a frame to itself


def block_inputs(seed=7):
    rng = np.random.default_rng(seed)
    fmaps = dev(rng.standard_normal((1, 5, 32, 8, 12)), torch.float16)
    yy, xx = np.meshgrid(np.arange(8.0), np.arange(12.0), indexing="ij")
    coords = np.stack([xx, yy], -1)[None, None] + rng.uniform(-3, 3, (1, len(II), 8, 12, 2))
    return fmaps, dev(coords, torch.float32), dev(np.array(II)), dev(np.array(JJ))


def test_block_matches_the_oracle_and_the_plain_op_per_level():
    import droid_backends
    from wgsr.frontend import AltCorrBlock
    fmaps, coords, ii, jj = block_inputs()
    block = AltCorrBlock(fmaps, num_levels=LEVELS, radius=RADIUS)
    out = block(coords, ii, jj)
    rd2 = (2 * RADIUS + 1) ** 2
    assert tuple(out.shape) == (1, len(II), LEVELS * rd2, 8, 12)
    assert out.dtype == torch.float32 and out.is_contiguous() and not out.requires_grad
    got = out.cpu().numpy()
    entry_coords = coords[0][:, None].contiguous()  # [E, 1, H, W, 2]
    for i, level in enumerate(block.pyramid):
        assert tuple(level.shape) == (1, 5, 8 // 2 ** i, 12 // 2 ** i, 32) and level.dtype == torch.float16
        f1, f2 = block.pyramid[0][0, ii], level[0, jj]
        ref, mag = A.altcorr_forward(f1.cpu().numpy(), f2.cpu().numpy(), entry_coords.cpu().numpy(), RADIUS,
                                     scale=2.0 ** -i)
        bound = A.forward_bound(mag, 32)[:, 0]
        mine = got[0][:, i * rd2:(i + 1) * rd2]
        check(f"level {i}", mine, ref[:, 0], bound)
        plain, = droid_backends.altcorr_forward(f1.float().contiguous(), f2.float().contiguous(),
                                                (entry_coords / 2 ** i).contiguous(), RADIUS)
        check(f"level {i} against the plain op", mine, plain[:, 0].double().cpu().numpy(), 2 * bound)


def test_block_with_samples_and_batches():
    from wgsr.frontend import AltCorrBlock
    fmaps, coords, ii, jj = block_inputs()
    block = AltCorrBlock(fmaps, num_levels=LEVELS, radius=RADIUS)
    shifted = coords + 0.37
    out = torch.stack([block(coords, ii, jj), block(shifted, ii, jj)], -1)
    sampled = block(torch.stack([coords, shifted], -2), ii, jj)
    assert tuple(sampled.shape) == (1, len(II), LEVELS * 49, 8, 12, 2)
    assert sampled.dtype == torch.float32 and sampled.is_contiguous()
    assert torch.equal(sampled, out)  # (the forward is bit-reproducible)
    # two batches: batch b reads map b N + ii
    other = block_inputs(seed=8)[0]
    both = AltCorrBlock(torch.cat([fmaps, other]), num_levels=LEVELS, radius=RADIUS)
    got = both(torch.cat([coords, shifted]), ii, jj)
    assert torch.equal(got[0], out[0, ..., 0])
    assert torch.equal(got[1], AltCorrBlock(other, num_levels=LEVELS, radius=RADIUS)(shifted, ii, jj)[0])


def test_block_allocates_only_its_output():
    from wgsr.frontend import AltCorrBlock
    fmaps, coords, ii, jj = block_inputs()
    block = AltCorrBlock(fmaps, num_levels=LEVELS, radius=RADIUS)
    block(coords, ii, jj)  # (the library is loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = block(coords, ii, jj)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print("peak growth", grew, "output", out.numel() * 4, "coords", coords.numel() * 4)
    # no per-edge copies of the maps (each would be 6 x 8 x 12 x 32 elements)
    assert grew <= out.numel() * 4 + coords.numel() * 4
