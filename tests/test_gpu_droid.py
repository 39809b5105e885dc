"""GPU tests of the ``droid_backends`` kernels (csrc/droid.hip) and of
``wgsr.frontend`` against the float64 oracle of tests/_droid_ref.py.

Tolerances.  depth_filter counts are integers: exact off the borderline
pixels the oracle flags (tests/test_droid_ref.py caps their share).
frame_distance: 1e-4 relative per pair, the project's fp32 contract for sums
of about 10^3 terms.  iproj: 1e-5 of each point's largest coordinate (the
rotation mixes the coordinates, so an element's error scales with the point,
not with the element).  Lookup: |d| <= tol |ref| + 1e-6 max|input| with tol =
1e-5 (fp32) or 2^-10 (fp16, one rounding of the fp32 sum; the oracle reads the
fp16-rounded input); at most four products of weights summing to one
accumulate, so the fp32 sum is within 4 x 2^-24 max|input| of exact.
"""
import functools

import numpy as np
import pytest
import torch

import _droid_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def frames():
    poses, disps, intr = R.make_inputs()
    return poses, disps, intr, dev(poses), dev(disps), dev(intr)


@functools.lru_cache(maxsize=None)
def filter_ref(inds):
    poses, disps, intr = R.make_inputs()
    n = R.NFRAMES
    th = R.filter_thresh(disps[:n], list(inds))
    count, border = R.depth_filter(poses[:n], disps[:n], intr, list(inds), th)
    return th, count, border


# ---------------------------------------------------------------------------
# depth_filter
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("inds", [tuple(range(R.NFRAMES)), (7, 2, 4)])
def test_depth_filter_counts_are_exact(inds):
    import droid_backends
    _, _, _, poses, disps, intr = frames()
    n = R.NFRAMES
    th, ref, border = filter_ref(inds)
    count = droid_backends.depth_filter(poses[:n].contiguous(), disps[:n].contiguous(), intr,
                                        dev(np.array(inds, np.int64)), dev(th))
    assert count.shape == (len(inds), R.HT, R.WD) and count.dtype == torch.float32
    got = count.cpu().numpy()
    bad = (got != ref) & ~border
    print("borderline", int(border.sum()), "differ on borderline", int(((got != ref) & border).sum()),
          "differ elsewhere", int(bad.sum()))
    assert not bad.any()
    assert border.mean() <= 0.02


# ---------------------------------------------------------------------------
# frame_distance
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def distance_ref():
    poses, disps, intr = R.make_inputs()
    n = len(poses)
    ii, jj = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    dist, ratio, near = R.frame_distance(poses, disps, intr, ii, jj, R.BETA)
    return ii, jj, dist, near


def test_frame_distance_matches_the_oracle():
    import droid_backends
    _, _, _, poses, disps, intr = frames()
    ii, jj, ref, near = distance_ref()
    got = droid_backends.frame_distance(poses, disps, intr, dev(ii, torch.int64), dev(jj, torch.int64), R.BETA)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == (144,) and np.isfinite(got).all()
    far = ref == 1000
    assert (got[far] == 1000).all()
    check = ~far & ~near
    err = np.abs(got - ref)[check] / np.maximum(np.abs(ref[check]), 1e-300)
    err[(got[check] == 0) & (ref[check] == 0)] = 0
    print("pairs checked", int(check.sum()), "worst relative error", err.max())
    assert check.sum() >= 100 and near.sum() <= 14
    assert (np.abs(got - ref)[check] <= 1e-4 * np.abs(ref[check])).all()


def test_fused_bidirectional_is_the_mean_of_the_two_calls():
    import droid_backends
    from wgsr import frontend
    _, _, _, poses, disps, intr = frames()
    ii, jj, _, _ = distance_ref()
    di, dj = dev(ii, torch.int64), dev(jj, torch.int64)
    d1 = droid_backends.frame_distance(poses, disps, intr, di, dj, R.BETA).cpu().numpy().astype(np.float64)
    d2 = droid_backends.frame_distance(poses, disps, intr, dj, di, R.BETA).cpu().numpy().astype(np.float64)
    both = frontend.distance(poses, disps, intr, di, dj, beta=R.BETA).cpu().numpy().astype(np.float64)
    mean = 0.5 * (d1 + d2)
    assert (np.abs(both - mean) <= 1e-6 * np.abs(mean)).all()
    # the matrix form, and the one-way form through the same entry
    mat = frontend.distance(poses, disps, intr, beta=R.BETA)
    assert mat.shape == (12, 12) and np.array_equal(mat.cpu().numpy().ravel().astype(np.float64), both)
    one = frontend.distance(poses, disps, intr, di, dj, beta=R.BETA, bidirectional=False)
    assert np.array_equal(one.cpu().numpy().astype(np.float64), d1)


# ---------------------------------------------------------------------------
# iproj
# ---------------------------------------------------------------------------
def test_iproj_matches_the_oracle():
    import droid_backends
    hp, hd, hi, poses, disps, intr = frames()
    n = R.NFRAMES
    got = droid_backends.iproj(poses[:n].contiguous(), disps[:n].contiguous(), intr)
    assert got.shape == (n, R.HT, R.WD, 3)
    ref = R.iproj(hp[:n], hd[:n], hi)
    err = np.abs(got.cpu().numpy() - ref).max(-1) / np.abs(ref).max(-1)
    print("iproj worst relative error", err.max())
    assert err.max() <= 1e-5


# ---------------------------------------------------------------------------
# corr_index
# ---------------------------------------------------------------------------
# (n, h1, w1, h2, w2, r): a small odd shape at both radii; then one whose
# planes take the 16-byte store path of the backward (w2 a multiple of 8) with
# more than one workgroup per volume and a partial last one (72 positions)
LOOKUP_CASES = [(3, 5, 7, 6, 9, 3), (3, 5, 7, 6, 9, 1), (2, 9, 8, 5, 16, 2)]
TOL = {torch.float32: 1e-5, torch.float16: 2.0 ** -10}


@functools.lru_cache(maxsize=None)
def lookup_ref(case, half):
    n, h1, w1, h2, w2, r = case
    volume, coords = R.make_lookup_inputs(n, h1, w1, h2, w2)
    rd = 2 * r + 1
    grad_out = np.random.default_rng(11).standard_normal((n, rd, rd, h1, w1))
    if half:  # the oracle reads what the kernel reads
        volume = volume.astype(np.float16).astype(np.float64)
        grad_out = grad_out.astype(np.float16).astype(np.float64)
    else:
        volume = volume.astype(np.float32).astype(np.float64)
        grad_out = grad_out.astype(np.float32).astype(np.float64)
    fwd = R.corr_index_forward(volume, coords, r)
    bwd, touched = R.corr_index_backward(volume.shape, coords, grad_out, r)
    return volume, coords, grad_out, fwd, bwd, touched


def close(got, ref, tol, scale):
    d = np.abs(got.astype(np.float64) - ref)
    bound = tol * np.abs(ref) + 1e-6 * scale
    print("worst |d| / bound", (d / bound).max())
    return (d <= bound).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", LOOKUP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_corr_index_forward_and_backward(case, dtype):
    import droid_backends
    n, h1, w1, h2, w2, r = case
    volume, coords, grad_out, fwd, bwd, touched = lookup_ref(case, dtype == torch.float16)
    scale = min(np.abs(volume).max(), np.abs(grad_out).max())
    v, c, g = dev(volume, dtype), dev(coords), dev(grad_out, dtype)
    out = droid_backends.corr_index_forward(v, c, r)
    assert isinstance(out, list) and len(out) == 1
    corr = out[0]
    assert corr.shape == (n, 2 * r + 1, 2 * r + 1, h1, w1) and corr.dtype == dtype
    assert close(corr.float().cpu().numpy(), fwd, TOL[dtype], scale)
    out = droid_backends.corr_index_backward(v, c, g, r)
    assert isinstance(out, list) and len(out) == 1
    vg = out[0]
    assert vg.shape == v.shape and vg.dtype == dtype
    vg = vg.float().cpu().numpy()
    assert close(vg, bwd, TOL[dtype], scale)
    assert (vg[~touched] == 0).all() and (~touched).any()


class _Lookup(torch.autograd.Function):
    """The shape of the call the tracker's sampler makes: forward saves the
    volume and the coordinates, backward hands back one gradient."""

    @staticmethod
    def forward(ctx, volume, coords, radius):
        import droid_backends
        ctx.radius = radius
        ctx.save_for_backward(volume, coords)
        return droid_backends.corr_index_forward(volume, coords, radius)[0]

    @staticmethod
    def backward(ctx, grad):
        import droid_backends
        volume, coords = ctx.saved_tensors
        return droid_backends.corr_index_backward(volume, coords, grad.contiguous(), ctx.radius)[0], None, None


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_corr_index_through_autograd(dtype):
    case = LOOKUP_CASES[0]
    r = case[-1]
    volume, coords, grad_out, fwd, bwd, touched = lookup_ref(case, dtype == torch.float16)
    scale = min(np.abs(volume).max(), np.abs(grad_out).max())
    v = dev(volume, dtype).requires_grad_(True)
    corr = _Lookup.apply(v, dev(coords), r)
    assert close(corr.detach().float().cpu().numpy(), fwd, TOL[dtype], scale)
    # a non-contiguous upstream gradient, as autograd may hand over
    g = dev(grad_out, dtype).permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)
    corr.backward(g)
    vg = v.grad.float().cpu().numpy()
    assert close(vg, bwd, TOL[dtype], scale)
    assert (vg[~touched] == 0).all()


# ---------------------------------------------------------------------------
# wgsr.frontend
# ---------------------------------------------------------------------------
def test_valid_depth_mask_matches_the_oracle_pipeline():
    import droid_backends
    from wgsr import frontend
    _, hd, _, poses, disps, intr = frames()
    n = R.NFRAMES
    inds = tuple(range(n))
    th, ref_count, border = filter_ref(inds)
    # a borderline count sitting at visible_num may fall on either side
    excl = border & ((ref_count == R.VISIBLE_NUM) | (ref_count == R.VISIBLE_NUM - 1))
    assert excl.mean() <= 0.02
    ref_mask, _ = R.valid_depth_mask(hd[:n], list(inds), ref_count)
    p, d = poses[:n].contiguous(), disps[:n].contiguous()
    idx = dev(np.array(inds, np.int64))
    mask = frontend.valid_depth_mask(p, d, intr, idx, thresh=R.FILTER_THRESH, visible_num=R.VISIBLE_NUM)
    assert mask.shape == (n, R.HT, R.WD) and mask.dtype == torch.bool
    got = mask.cpu().numpy()
    print("excluded", int(excl.sum()), "differ", int((got != ref_mask).sum()))
    assert np.array_equal(got[~excl], ref_mask[~excl])
    assert 0.2 < got.mean() < 1.0
    # the medians, with the excluded pixels left out on both sides
    _, ref_med = R.valid_depth_mask(hd[:n], list(inds), ref_count, exclude=excl)
    depths = 1.0 / d
    thr = (R.FILTER_THRESH * depths.mean(dim=[1, 2])).contiguous()
    assert np.abs(thr.cpu().numpy() - th).max() <= 1e-6 * th.max()
    count = droid_backends.depth_filter(p, d, intr, idx, thr)
    depths[~(count >= R.VISIBLE_NUM) | dev(excl)] = torch.nan
    med = depths.view(n, -1).nanmedian(dim=1).values.cpu().numpy().astype(np.float64)
    assert (np.abs(med - ref_med) <= 1e-6 * ref_med).all()
    # no neighbour agrees (threshold 0): an all-False mask
    none = frontend.valid_depth_mask(p, d, intr, idx, thresh=0.0, visible_num=R.VISIBLE_NUM)
    assert not none.any()


def test_depth_and_pose():
    from wgsr import frontend
    hp, hd, _, poses, disps, _ = frames()
    f = 5
    q, t = hp[f, 3:].astype(np.float64), hp[f, :3].astype(np.float64)
    w2c = np.eye(4)
    w2c[:3, :3] = np.stack([R.rotate(q, e) for e in np.eye(3)], 1)
    w2c[:3, 3] = t
    mask = torch.zeros(R.HT, R.WD, dtype=torch.bool, device=DEV)
    mask.view(-1)[:100] = True
    depth, m, c2w, invalid = frontend.depth_and_pose(poses[f], disps[f], mask)
    assert not invalid and torch.equal(m, mask)
    assert np.abs(c2w.cpu().numpy().astype(np.float64) @ w2c - np.eye(4)).max() <= 1e-6
    assert np.abs(depth.cpu().numpy() - 1.0 / hd[f].astype(np.float64)).max() <= 1e-6 * (1.0 / hd[f]).max()
    mask.view(-1)[99] = False
    assert frontend.depth_and_pose(poses[f], disps[f], mask)[3]
