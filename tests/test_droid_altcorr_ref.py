"""CPU tests of ``droid_backends.altcorr_*`` and ``wgsr.frontend.AltCorrBlock``
(no GPU needed): the float64 oracle (tests/_droid_altcorr_ref.py) against
independent statements of the op, the conditions its inputs must meet for the
GPU tests (tests/test_gpu_droid_altcorr.py) to be decisive, the room a plain
fp32 evaluation leaves inside the GPU bound, the pyramid, and the module
surface."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _droid_altcorr_ref as A
import _droid_ref as R

CASES = range(len(A.SHAPES))


def _volume(case):
    return np.einsum("bhwc,byxc->bhwyx", case["fmap1"].astype(np.float64), case["fmap2"].astype(np.float64))


@pytest.mark.parametrize("index", CASES)
def test_forward_oracle_is_the_lookup_of_the_all_pairs_volume(index):
    case = A.forward_case(index)
    B, N, H1, W1 = case["coords"].shape[:4]
    rd = 2 * case["r"] + 1
    assert case["corr"].shape == (B, N, rd * rd, H1, W1)
    volume = _volume(case)
    for n in range(N):
        coords = np.moveaxis(case["coords"][:, n], -1, 1)  # [B, 2, H1, W1]
        ref = R.corr_index_forward(volume, coords, case["r"]).reshape(B, rd * rd, H1, W1)
        assert np.abs(case["corr"][:, n] - ref).max() <= 1e-12


def _torch_composition(fmap1, fmap2, coords, r):
    """all-pairs einsum + the lookup stated with F.grid_sample (zero padding,
    align_corners), differentiable, float64: [B, N, (2r+1)^2, H1, W1]."""
    B, N, H1, W1, _ = coords.shape
    H2, W2 = fmap2.shape[1:3]
    rd = 2 * r + 1
    volume = torch.einsum("bhwc,byxc->bhwyx", fmap1, fmap2).reshape(B * H1 * W1, 1, H2, W2)
    off = torch.arange(-r, r + 1, dtype=torch.float64)
    delta = torch.stack(torch.meshgrid(off, off, indexing="ij"), -1).reshape(1, rd, rd, 2)  # [ix, iy] -> (x, y)
    out = []
    for n in range(N):
        g = coords[:, n].reshape(B * H1 * W1, 1, 1, 2) + delta
        g = torch.stack([2 * g[..., 0] / (W2 - 1) - 1, 2 * g[..., 1] / (H2 - 1) - 1], -1)
        s = F.grid_sample(volume, g, mode="bilinear", padding_mode="zeros", align_corners=True)
        out.append(s.reshape(B, H1, W1, rd * rd).permute(0, 3, 1, 2))
    return torch.stack(out, 1)


@pytest.mark.parametrize("index", CASES)
def test_backward_oracle_is_autograd_of_the_composition(index):
    case = A.backward_case(index)
    f1 = torch.from_numpy(case["fmap1"].astype(np.float64)).requires_grad_()
    f2 = torch.from_numpy(case["fmap2"].astype(np.float64)).requires_grad_()
    coords = torch.from_numpy(case["coords"].astype(np.float64))
    corr = _torch_composition(f1, f2, coords, case["r"])
    assert np.abs(corr.detach().numpy() - case["corr"]).max() <= 1e-11
    corr.backward(torch.from_numpy(case["corr_grad"].astype(np.float64)))
    # grid_sample goes through normalised coordinates: a few float64 roundings
    # of the weights, relative to each sum's magnitude
    assert (np.abs(f1.grad.numpy() - case["fmap1_grad"]) <= 1e-12 * (1 + case["mag1"])).all()
    assert (np.abs(f2.grad.numpy() - case["fmap2_grad"]) <= 1e-12 * (1 + case["mag2"])).all()
    assert (case["fmap2_grad"][~case["touched"]] == 0).all()


@pytest.mark.parametrize("index", CASES)
def test_inputs_are_decisive(index):
    case = A.backward_case(index)
    assert np.isfinite(case["coords"]).all()
    assert (case["corr"] != 0).mean() >= 0.5
    assert (case["mag"] == 0).any()            # windows wholly outside the plane
    assert case["touched"].any() and (~case["touched"]).any()
    assert case["count"].max() > 16            # the count term of the bound matters


def _fp32_forward(case):
    """The op evaluated in float32 the plain way: every dot product summed
    channel by channel, then the four-term blend."""
    f1, f2, coords, r = case["fmap1"], case["fmap2"], case["coords"], case["r"]
    B, N, H1, W1, _ = coords.shape
    H2, W2, C = f2.shape[1:]
    rd = 2 * r + 1
    volume = np.zeros((B, H1, W1, H2 + 2, W2 + 2), np.float32)  # (one ring of zeros: taps outside the plane)
    inner = volume[:, :, :, 1:-1, 1:-1]
    for c in range(C):
        inner += f1[:, :, :, None, None, c] * f2[:, None, None, :, :, c]
    out = np.zeros((B, N, rd * rd, H1, W1), np.float32)
    one = np.float32(1)
    for b in range(B):
        for n in range(N):
            for y in range(H1):
                for x in range(W1):
                    x0, y0 = coords[b, n, y, x]
                    fx, fy = np.floor(x0), np.floor(y0)
                    dx, dy = np.float32(x0 - fx), np.float32(y0 - fy)
                    for ix in range(rd):
                        for iy in range(rd):
                            X, Y = int(fx) + ix - r, int(fy) + iy - r
                            q = [volume[b, y, x, min(max(Y + oy, -1), H2) + 1, min(max(X + ox, -1), W2) + 1]
                                 for oy in (0, 1) for ox in (0, 1)]
                            out[b, n, iy + rd * ix, y, x] = ((one - dx) * (one - dy) * q[0] + dx * (one - dy) * q[1]
                                                             + (one - dx) * dy * q[2] + dx * dy * q[3])
    return out


def test_plain_fp32_evaluation_is_well_inside_the_gpu_bound():
    case = A.forward_case(0)
    got = _fp32_forward(case).astype(np.float64)
    bound = A.forward_bound(case["mag"], case["C"])
    err = np.abs(got - case["corr"])
    assert (got[case["mag"] == 0] == 0).all()
    live = bound > 0
    print("worst error / bound", (err[live] / bound[live]).max())
    assert (err <= bound).all()
    assert (err[live] / bound[live]).max() <= 0.25


def test_pyramid_matches_float64_pooling():
    from wgsr.frontend import AltCorrBlock
    fmaps = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 5, 32, 8, 12))).to(torch.float16)
    block = AltCorrBlock(fmaps, num_levels=4, radius=3)
    assert block.num_levels == 4 and block.radius == 3 and len(block.pyramid) == 4
    ref = fmaps.double().reshape(5, 32, 8, 12) / 4.0  # (exact in fp16 too, but for the subnormals)
    mag = ref.abs()
    for i, level in enumerate(block.pyramid):
        assert level.dtype == torch.float16 and level.is_contiguous()
        assert tuple(level.shape) == (1, 5, 8 // 2 ** i, 12 // 2 ** i, 32)
        got = level.double().reshape(5, 8 // 2 ** i, 12 // 2 ** i, 32).permute(0, 3, 1, 2)
        # one fp16 rounding (2^-11 relative, 2^-25 in the subnormals) per pooling step
        assert ((got - ref).abs() <= i * 2.0 ** -11 * mag + (i + 1) * 2.0 ** -25).all()
        if i + 1 < 4:
            ref, mag = F.avg_pool2d(ref, 2, stride=2), F.avg_pool2d(mag, 2, stride=2)


def _host_inputs(c=64, dtype=torch.float32):
    return (torch.zeros(2, 4, 5, c, dtype=dtype), torch.zeros(2, 3, 6, c, dtype=dtype), torch.zeros(2, 1, 4, 5, 2))


def test_host_tensors_never_reach_a_kernel():
    import droid_backends
    from wgsr.frontend import AltCorrBlock
    f1, f2, coords = _host_inputs()
    with pytest.raises(RuntimeError, match="HIP device"):
        droid_backends.altcorr_forward(f1, f2, coords, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        droid_backends.altcorr_forward(f1.half(), f2.half(), coords, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        droid_backends.altcorr_backward(f1, f2, coords, torch.zeros(2, 1, 49, 4, 5), 3)
    block = AltCorrBlock(torch.zeros(1, 3, 32, 4, 6, dtype=torch.float16), num_levels=2)
    with pytest.raises(RuntimeError, match="HIP device"):
        block(torch.zeros(1, 2, 4, 6, 2), torch.tensor([0, 1]), torch.tensor([1, 2]))


def test_argument_checks():
    import droid_backends
    f1, f2, coords = _host_inputs()
    with pytest.raises(RuntimeError, match="fmap2 must be contiguous"):
        droid_backends.altcorr_forward(f1, torch.zeros(2, 6, 3, 64).transpose(1, 2), coords, 3)
    with pytest.raises(RuntimeError, match="coords must be contiguous"):
        droid_backends.altcorr_forward(f1, f2, torch.zeros(2, 1, 5, 4, 2).transpose(2, 3), 3)
    with pytest.raises(RuntimeError, match="corr_grad must be contiguous"):
        droid_backends.altcorr_backward(f1, f2, coords, torch.zeros(2, 1, 49, 5, 4).transpose(3, 4), 3)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        droid_backends.altcorr_forward(*_host_inputs(c=24), 3)
    with pytest.raises(RuntimeError, match="float32 or float16"):
        droid_backends.altcorr_forward(*_host_inputs(dtype=torch.float64), 3)
    g1, g2, c = _host_inputs(dtype=torch.float16)
    with pytest.raises(RuntimeError, match="must both be float32"):
        droid_backends.altcorr_backward(g1, g2, c, torch.zeros(2, 1, 49, 4, 5, dtype=torch.float16), 3)
    with pytest.raises(RuntimeError, match="coords must be a float32 tensor"):
        droid_backends.altcorr_forward(f1, f2, torch.zeros(2, 1, 4, 5), 3)


def test_only_the_reference_call_forms():
    import droid_backends
    for name in ("altcorr_forward", "altcorr_backward", "projmap"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(droid_backends, name)()
    f1, f2, coords = _host_inputs()
    with pytest.raises(NotImplementedError, match=r"\(fmap1, fmap2, coords, radius\)"):
        droid_backends.altcorr_forward(f1, f2, coords, radius=3)
    with pytest.raises(NotImplementedError, match=r"\(fmap1, fmap2, coords, corr_grad, radius\)"):
        droid_backends.altcorr_backward(f1, f2, coords, 3)
