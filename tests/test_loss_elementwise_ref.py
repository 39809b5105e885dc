"""CPU checks of tests/_loss_elementwise_ref.py (no GPU): every case stays
inside its masking cap and reaches what it was picked for, the fp32
restatement passes the bound with margin 1 (by construction), and single
corruptions of the restatement -- of the kind a whole-tensor rel-L1 lets
through -- fail the element-wise check."""
import copy

import numpy as np
import pytest
import torch

import _loss_elementwise_ref as E

SSIM_ALL = E.ssim_case_names()
# the seam corruptions need a second tile column and a second tile row
SSIM_SEAM = [n for n in SSIM_ALL if E.ssim_case(n).shape[-2] > 16 and E.ssim_case(n).shape[-1] > 64]
MLP_ALL = list(E.MLP_CASES)
UNC_ALL = list(E.UNC_CASES)


def _mutated(o32, k, f):
    got = copy.copy(o32)
    got[k] = np.array(o32[k], np.float64, copy=True)
    f(got[k])
    return got


def _rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))


# --------------------------------------------------------------------- SSIM

def test_ssim_restatement_statistics_are_the_oracles():
    """ssim_stats restates oracle.ssim._stats: in float64 with the oracle's
    own window it gives the same numbers."""
    c = E.ssim_case("3x33x129-w7-flat")
    a, b = c.ren.numpy()[1], c.gt.numpy()[1]
    for mine, theirs in zip(E.ssim_stats(a, b, 7, np.float64, w2d=E.osim.window_2d(7)), E.osim._stats(a, b, 7)):
        np.testing.assert_array_equal(mine, theirs)
    S, _ = E.ssim_maps(E.osim._stats(a, b, 7), np.float64)
    np.testing.assert_allclose(S, E.osim.ssim_map_f64(a, b, 7), rtol=1e-14)


def test_ssim_derivative_maps_are_the_gradient():
    """The three maps pushed through the window's adjoint are the float64
    autograd gradient of ssim_torch: dL/dx = s (W*d0 + 2 x W*d1 + y W*d2)."""
    c = E.ssim_case("1x17x65-w5-textured")
    x, y = c.ren.numpy()[0].astype(np.float64), c.gt.numpy()[0].astype(np.float64)
    w = E.osim.window_2d(5)
    conv = [E.osim.conv_same(c.o64[f"dmap{i}"][0], w) for i in range(3)]
    grad = -(conv[0] + 2 * x * conv[1] + y * conv[2]) / x.size
    np.testing.assert_allclose(grad, c.o64["grad"][0], rtol=0, atol=1e-12 * np.abs(grad).max())


def test_ssim_flat_images_reach_the_floors():
    c = E.ssim_case("3x33x129-w11-flat")
    # a window wholly inside a constant patch (the fp32 window's weights sum to
    # 1 + O(1e-7), which is all the variance that is left there)
    assert c.var.min() < 1e-6 and c.var.max() > 0.05
    t = E.ssim_case("3x33x129-w11-textured")
    assert np.abs(c.o64["dmap1"]).max() > 3 * np.abs(t.o64["dmap1"]).max()
    assert float(c.gt[..., 0, :].abs().max()) == 0 and float(c.ren[..., 0, :].abs().max()) > 0  # black border
    assert float((c.gt == 1).float().mean()) > 0.03 and float((c.ren == 1).float().mean()) > 0.03


@pytest.mark.parametrize("name", SSIM_ALL)
def test_ssim_restatement_passes_with_margin_one(name):
    c = E.ssim_case(name)
    ratios = E.ssim_check(c, c.o32, margin=1)
    assert all(r <= 1.0 for r in ratios.values())


def _ssim_grad_mutants(c):
    yield "column 64 x 0.99", lambda g: g[:, :, 64].__imul__(0.99)
    yield "row 16 x 0.997", lambda g: g[:, 16, :].__imul__(0.997)
    yield "pixel (16, 64) x 0.5", lambda g: g[:, 16, 64].__imul__(0.5)
    if c.weights is not None:
        # image 0's first plane scaled by image 1's plane_scale
        yield "plane 0 under plane 3's scale", lambda g: g[0].__imul__(E.SSIM_WEIGHTS[1] / E.SSIM_WEIGHTS[0])


@pytest.mark.parametrize("name", SSIM_SEAM)
def test_ssim_gradient_corruptions_fail(name):
    c = E.ssim_case(name)
    for what, f in _ssim_grad_mutants(c):
        got = _mutated(c.o32, "grad", f)
        assert not np.array_equal(got["grad"], c.o32["grad"]), what
        with pytest.raises(AssertionError, match="grad"):
            E.ssim_check(c, got)


def test_ssim_stratification_is_what_catches_a_small_error_on_a_flat_image():
    """The flat patches raise the tensor's spread tens of times over a
    textured pixel's, so a 1 % error at the seam pixel passes the bound taken
    with the tensor's maxima; its variance group's maxima catch it."""
    c, t = E.ssim_case("2x3x35x70-w9-flat"), E.ssim_case("2x3x35x70-w9-textured")
    spread = lambda k: np.abs(k.o32["grad"] - k.o64["grad"]).max()  # noqa: E731
    assert spread(c) > 10 * spread(t)
    got = _mutated(c.o32, "grad", lambda g: g[:, 16, 64].__imul__(0.99))
    assert np.abs(got["grad"] - c.o64["grad"]).max() <= E.MARGIN * spread(c) + 1e-6 * np.abs(c.o64["grad"]).max()
    with pytest.raises(AssertionError, match="grad group"):
        E.ssim_check(c, got)


def test_ssim_seam_corruptions_pass_todays_rel_l1():
    """The gap: tests/test_gpu_ssim.py's rel-L1 <= 1e-4 lets the scaled seam
    column and the scaled seam row through even on this small frame (a single
    pixel's share of the sum falls under it from about 3 x 70 x 130 on)."""
    c = E.ssim_case("3x33x129-w11-textured")
    for what, f in list(_ssim_grad_mutants(c))[:2]:
        got = _mutated(c.o32, "grad", f)
        assert _rel_l1(got["grad"], c.o64["grad"]) <= 1e-4, what


@pytest.mark.parametrize("name", SSIM_SEAM)
def test_ssim_dropped_halo_tap_fails(name):
    """Column 64 (the first of the second tile column) recomputed with the
    window's first horizontal tap zeroed: the tap that comes from the
    neighbouring tile's side of the seam."""
    c = E.ssim_case(name)
    w = E.osim.window_2d(c.ws).copy()
    w[:, 0] = 0
    a = c.ren.numpy().reshape(-1, *c.shape[-2:])
    b = c.gt.numpy().reshape(-1, *c.shape[-2:])
    got = copy.copy(c.o32)
    for i in range(3):
        got[f"dmap{i}"] = c.o32[f"dmap{i}"].copy()
    for p in range(a.shape[0]):
        _, d = E.ssim_maps(E.ssim_stats(a[p], b[p], c.ws, np.float32, w2d=w), np.float32)
        for i in range(3):
            got[f"dmap{i}"][p, :, 64] = d[i][:, 64]
    with pytest.raises(AssertionError, match="dmap0.*dmap1.*dmap2"):
        E.ssim_check(c, got)


# ---------------------------------------------------------------------- MLP

@pytest.mark.parametrize("name", MLP_ALL + ["seg2"])
def test_mlp_caps_and_restatement(name):
    c = E.mlp_seg2_case() if name == "seg2" else E.mlp_case(name)
    print(f"{c.name}: {int(c.near.sum())} near rows of {c.near.size}")
    assert c.near.mean() <= E.MAX_MASKED
    ratios = E.mlp_check(c, c.o32, margin=1)
    assert all(r <= 1.0 for r in ratios.values())
    assert all(np.abs(c.o64[k]).max() > 0 for k in E.MLP_PARAMS)


def test_mlp_cases_reach_their_kernels():
    """The dispatch conditions of csrc/mlp.hip, restated on the shapes."""
    def small(N, C, aligned):
        return aligned and (N + 63) // 64 < 1024 and C in (64, 128, 256, 384)

    def fwd(N, C, aligned):
        return "small" if small(N, C, aligned) else ("fwd64" if (N + 63) // 64 >= 1024 else "fwd16")

    def bwd(N, C, aligned):
        return "bwd2" if aligned and ((N + 63) // 64) * (C // 64) <= 1024 else "bwd"
    want = {"1275x384": ("small", "bwd2"), "17x64": ("small", "bwd2"), "1x64": ("small", "bwd2"),
            "300x256": ("small", "bwd2"), "1000x192": ("fwd16", "bwd2"), "65600x64": ("fwd64", "bwd"),
            "1275x384-offset4": ("fwd16", "bwd")}
    for name, (N, C, p, mis, _) in E.MLP_CASES.items():
        assert (fwd(N, C, not mis), bwd(N, C, not mis)) == want[name], name
    N = 65600
    assert (N + 63) // 64 == 1025 and ((N + 63) // 64 + 15) // 16 == 65 and ((N + 63) // 64) % 16 == 1
    assert 1275 % 16 and 1275 % 64 and 17 % 16


def _mlp_mutants(c):
    yield "u", "one row of u x 1.005", lambda o: _mutated(o, "u", lambda u: u[c.N // 2:c.N // 2 + 1].__imul__(1.005))
    if c.C >= 128:
        yield "dW1", "columns 64..127 of dW1 x (1 + 1e-4)", \
            lambda o: _mutated(o, "dW1", lambda g: g[:, 64:128].__imul__(1 + 1e-4))
    last = int(np.flatnonzero(~c.near)[-1])
    du = c.du.clone()
    du[last] = 0
    dropped = E.mlp_run(c, torch.float32, du=du)
    yield "d[Wb][123]", "the last row's contribution dropped", lambda o: {**dropped, "u": o["u"]}


@pytest.mark.parametrize("name", MLP_ALL)
def test_mlp_corruptions_fail(name):
    c = E.mlp_case(name)
    for match, what, f in _mlp_mutants(c):
        with pytest.raises(AssertionError, match=match):
            E.mlp_check(c, f(c.o32))
    # ... the dropped row in every gradient tensor on its own
    last = int(np.flatnonzero(~c.near)[-1])
    du = c.du.clone()
    du[last] = 0
    dropped = E.mlp_run(c, torch.float32, du=du)
    for k in E.MLP_PARAMS:
        with pytest.raises(AssertionError, match=k):
            E.mlp_check(c, {**c.o32, k: dropped[k]})


# -------------------------------------------------- uncertainty mapping loss

@pytest.mark.parametrize("name", UNC_ALL)
def test_uncer_caps_census_and_restatement(name):
    c = E.unc_case(name)
    print(f"{name}: {int(c.near.sum())} of {c.near.size} pixels and {int(c.near_clip.sum())} of "
          f"{c.near_clip.size} small pixels excluded")
    assert c.near.mean() <= E.MAX_MASKED
    assert c.near_clip.mean() <= E.MAX_MASKED and c.near_small.mean() <= E.MAX_MASKED
    for k, m in c.census.items():
        assert m.any() and not m.all(), f"{k} has one outcome only"
    for k in E.UNC_FULL + E.UNC_SMALL:
        assert np.all(np.isfinite(c.o64[k])) and np.abs(c.o64[k]).max() > 0, k
    ratios = E.unc_check(c, c.o32, margin=1)
    assert all(r <= 1.0 for r in ratios.values())
    if c.init:
        assert c.o64["d_exposure_a"] is None and c.o64["d_exposure_b"] is None


def test_uncer_no_decision_flips_in_the_restatement():
    """The fp32 restatement takes every mask the way float64 does off the
    near pixels, so its spread is rounding alone."""
    for name in UNC_ALL:
        c = E.unc_case(name)
        far = ~c.near
        for k in E.UNC_FULL:
            d = np.abs(c.o32[k] - c.o64[k])[:, far]
            assert d.max() <= 1e-4 * np.abs(c.o64[k]).max(), (name, k)


def _uncer_mutants(c):
    far = np.argwhere(~c.near)
    y, x = (int(v) for v in far[len(far) // 2])
    yield "d_image", "one d_image pixel x 0.5", _mutated(c.o32, "d_image", lambda g: g[:, y, x].__imul__(0.5))
    # (where the opacity mask zeroes both there is nothing to exchange)
    g64 = c.o64["d_unc"]
    keep = np.argwhere(~c.near_clip[:, :-1] & ~c.near_clip[:, 1:] & (g64[:, :-1] != g64[:, 1:]))
    i, j = (int(v) for v in keep[len(keep) // 2])

    def neighbour(g):
        g[i, j] = g[i, j + 1]
    yield "d_unc", "one d_unc entry taken from its neighbour", _mutated(c.o32, "d_unc", neighbour)
    # the whole run with the small map resampled one pixel off: its columns rolled
    t = dict(c.t)
    t["unc"] = torch.roll(c.t["unc"], 1, dims=1)
    off = E.unc_run(t, c.tf, c.sf, c.init, torch.float32)
    off["d_unc"] = np.roll(off["d_unc"], -1, axis=1)
    yield "d_image.*d_depth", "the small map's grid shifted by one pixel", off


@pytest.mark.parametrize("name", UNC_ALL)
def test_uncer_corruptions_fail(name):
    c = E.unc_case(name)
    for match, what, got in _uncer_mutants(c):
        with pytest.raises(AssertionError, match=match):
            E.unc_check(c, got)
