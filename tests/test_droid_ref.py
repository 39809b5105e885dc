"""CPU tests of the ``droid_backends`` drop-in (no GPU needed): the module
surface, the float64 oracle (tests/_droid_ref.py) against independent
statements of the same operations, and the conditions the shared inputs must
meet for the GPU tests (tests/test_gpu_droid.py) to be decisive."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _droid_ref as R

BUILT = ("frame_distance", "depth_filter", "iproj", "corr_index_forward", "corr_index_backward")
UNBUILT = ("ba", "projmap", "altcorr_forward", "altcorr_backward")


def test_module_exposes_the_reference_names():
    import droid_backends
    for name in BUILT + UNBUILT:
        assert callable(getattr(droid_backends, name)), name
    for name in UNBUILT:
        with pytest.raises(NotImplementedError, match=name):
            getattr(droid_backends, name)()


def test_contiguity_check_is_the_reference_message():
    import droid_backends
    poses, disps, intr = torch.zeros(3, 7), torch.ones(3, 4, 5), torch.ones(4)
    with pytest.raises(RuntimeError, match="disps must be contiguous"):
        droid_backends.iproj(poses, disps.transpose(1, 2), intr)
    with pytest.raises(RuntimeError, match="coords must be contiguous"):
        droid_backends.corr_index_forward(torch.zeros(1, 2, 3, 4, 5), torch.zeros(1, 3, 2, 2).transpose(1, 3), 1)
    # host tensors never reach a kernel
    with pytest.raises(RuntimeError, match="HIP device"):
        droid_backends.iproj(poses, disps, intr)


def _grid_sample_lookup(volume, coords, r):
    """The lookup stated with F.grid_sample (zero padding, align_corners):
    every position samples its own plane on its (2r+1)^2 window."""
    n, h1, w1, h2, w2 = volume.shape
    rd = 2 * r + 1
    v = torch.from_numpy(volume).reshape(n * h1 * w1, 1, h2, w2)
    c = torch.from_numpy(coords.astype(np.float64)).permute(0, 2, 3, 1).reshape(n * h1 * w1, 1, 1, 2)
    off = torch.arange(-r, r + 1, dtype=torch.float64)
    # window index i runs along x (first), j along y
    delta = torch.stack(torch.meshgrid(off, off, indexing="ij"), -1).reshape(1, rd, rd, 2)
    g = c + delta
    g = torch.stack([2 * g[..., 0] / (w2 - 1) - 1, 2 * g[..., 1] / (h2 - 1) - 1], -1)
    out = F.grid_sample(v, g, mode="bilinear", padding_mode="zeros", align_corners=True)
    return out.reshape(n, h1, w1, rd, rd).permute(0, 3, 4, 1, 2).numpy()


@pytest.mark.parametrize("r", [3, 1])
def test_lookup_oracle_agrees_with_grid_sample(r):
    volume, coords = R.make_lookup_inputs()
    ref = R.corr_index_forward(volume, coords, r)
    alt = _grid_sample_lookup(volume, coords, r)
    assert ref.shape == alt.shape == (3, 2 * r + 1, 2 * r + 1, 5, 7)
    assert np.abs(ref - alt).max() <= 1e-12


def test_lookup_inputs_cover_the_edge_cases():
    volume, coords = R.make_lookup_inputs()
    h2, w2 = volume.shape[3:]
    x, y = coords[:, 0].ravel().astype(np.float64), coords[:, 1].ravel().astype(np.float64)
    integer = (x == np.floor(x)) & (y == np.floor(y))
    inside = (x > 0) & (x < w2 - 1) & (y > 0) & (y < h2 - 1)
    assert (inside & ~integer).sum() >= 10 and (inside & integer).any()
    assert ((x > -1) & (x < 0)).any() and ((x > w2 - 1) & (x < w2)).any()
    assert ((y > -1) & (y < 0)).any() and ((y > h2 - 1) & (y < h2)).any()
    assert (x < 0).any() and (y < 0).any()
    # more than r + 1 outside (r = 3): the whole window is zero
    ref = R.corr_index_forward(volume, coords, 3)
    far = (x < -4) | (x > w2 + 3) | (y < -4) | (y > h2 + 3)
    assert far.sum() >= 4
    assert (np.abs(ref).reshape(3, 49, -1).max(1).ravel()[far] == 0).all()


@pytest.mark.parametrize("r", [3, 1])
def test_backward_oracle_is_the_adjoint(r):
    """<forward(V), G> == <V, backward(G)> and, the forward being linear in
    the volume, a finite difference of sum(forward(V) G) along a random
    direction equals <direction, backward(G)>."""
    volume, coords = R.make_lookup_inputs()
    rng = np.random.default_rng(7)
    G = rng.standard_normal(R.corr_index_forward(volume, coords, r).shape)
    grad, touched = R.corr_index_backward(volume.shape, coords, G, r)
    lhs = (R.corr_index_forward(volume, coords, r) * G).sum()
    assert abs(lhs - (volume * grad).sum()) <= 1e-10 * max(1.0, abs(lhs))
    direction = rng.standard_normal(volume.shape)
    eps = 1e-3
    fd = ((R.corr_index_forward(volume + eps * direction, coords, r)
           - R.corr_index_forward(volume - eps * direction, coords, r)) * G).sum() / (2 * eps)
    assert abs(fd - (direction * grad).sum()) <= 1e-8 * max(1.0, abs(fd))
    assert (grad[~touched] == 0).all() and touched.any() and (~touched).any()


def test_depth_filter_inputs_are_decisive():
    poses, disps, intr = R.make_inputs()
    n = R.NFRAMES
    inds = list(range(n))
    count, border = R.depth_filter(poses[:n], disps[:n], intr, inds, R.filter_thresh(disps[:n], inds))
    share = [float((count == k).mean()) for k in range(7)]
    print("count shares", [round(100 * s, 2) for s in share], "borderline", round(100 * float(border.mean()), 2))
    assert abs(sum(share) - 1) < 1e-12
    assert min(share) >= 0.03, share
    assert border.mean() <= 0.02


def test_frame_distance_inputs_are_decisive():
    poses, disps, intr = R.make_inputs()
    n = len(poses)
    assert n == 12
    ii, jj = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    dist, ratio, near = R.frame_distance(poses, disps, intr, ii, jj, R.BETA)
    print("min |ratio - 0.75|", np.abs(ratio - 0.75).min(), "near MIN_DEPTH", int(near.sum()))
    assert np.abs(ratio - 0.75).min() >= 0.05
    full, most = ratio > 0.999, (ratio >= 0.75) & (ratio <= 0.999)
    some, none = (ratio > 0) & (ratio < 0.75), ratio == 0
    assert full.sum() + most.sum() + some.sum() + none.sum() == len(ratio) == 144
    assert min(full.sum(), most.sum(), some.sum(), none.sum()) >= 5
    assert (dist[some | none] == 1000).all() and (dist[full | most] < 1000).all()
    assert near.sum() <= 0.10 * len(ratio)
    # a frame is at distance exactly 0 from itself
    assert (dist[ii == jj] == 0).all()


def test_valid_depth_mask_oracle_matches_torch_pipeline():
    """The oracle's mask and lower median against update_valid_depth_mask's
    torch statement (nanmedian), on the oracle's own count."""
    poses, disps, intr = R.make_inputs()
    n = R.NFRAMES
    inds = [7, 2, 4]
    count, _ = R.depth_filter(poses[:n], disps[:n], intr, inds, R.filter_thresh(disps[:n], inds))
    mask, med = R.valid_depth_mask(disps[:n], inds, count)
    depths = 1.0 / torch.from_numpy(disps[:n].astype(np.float64))[inds]
    depths[~(torch.from_numpy(count) >= R.VISIBLE_NUM)] = torch.nan
    tm = depths.view(3, -1).nanmedian(dim=1).values
    assert np.array_equal(tm.numpy(), med)
    assert np.array_equal((depths < 3 * tm[:, None, None]).numpy(), mask)
    assert 0.2 < mask.mean() < 1.0
    # no survivor: an all-False mask
    mask0, med0 = R.valid_depth_mask(disps[:n], inds, np.zeros_like(count))
    assert not mask0.any() and np.isnan(med0).all()
