"""CPU tests that pin the float64 SE3 / reprojection oracle (tests/_lie_ref.py)
to independent statements, without the lietorch drop-in:

* matrix(exp(xi)) = the matrix exponential of the 4 x 4 hat matrix
  (torch.linalg.matrix_exp), angles 0, 1e-9, 1e-5, 1e-2 (series branch), 1, 3;
* matrix(exp(tau)) = the reference's own SE3_exp (tests/golden/ref_helpers.npz);
* log inverts exp; the product is the matrix product; X X^-1 = identity;
* adj / adjT = central differences of log(X exp(eps a) X^-1);
* Ji, Jj, Jz of the reprojection = central differences of its coordinates
  under retr(pose_i, eps e_k), retr(pose_j, eps e_k) and disp + eps;
* the reprojection = the reference's projective_transform run over the
  oracle's group algebra (tests/golden/ref_reproject.npz);
* make_reproject_inputs() exercises both validity branches away from the
  thresholds.
"""
import os

import numpy as np
import pytest
import torch

import _lie_ref as lr
from _util import GOLDEN

THETAS = (0.0, 1e-9, 1e-5, 1e-2, 0.2, 0.3, 1.0, 3.0)


def _tangents(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for th in THETAS:
        for _ in range(4):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            out.append(np.concatenate([rng.normal(size=3), th * axis]))
    return np.stack(out)


def _hat(xi):
    M = np.zeros(xi.shape[:-1] + (4, 4))
    tx, ty, tz, a, b, c = (xi[..., k] for k in range(6))
    M[..., 0, 1], M[..., 0, 2], M[..., 1, 0] = -c, b, c
    M[..., 1, 2], M[..., 2, 0], M[..., 2, 1] = -a, -b, a
    M[..., 0, 3], M[..., 1, 3], M[..., 2, 3] = tx, ty, tz
    return M


def _elements(seed=1, n=12):
    rng = np.random.default_rng(seed)
    xi = rng.normal(size=(n, 6))
    xi[:, 3:] *= rng.uniform(0.0, 1.2, size=(n, 1))
    return lr.exp(xi)


def test_exp_is_the_matrix_exponential():
    xi = _tangents()
    ref = torch.linalg.matrix_exp(torch.from_numpy(_hat(xi))).numpy()
    got = lr.matrix(lr.exp(xi))
    assert np.abs(got - ref).max() <= 1e-12
    np.testing.assert_array_equal(lr.exp(np.zeros(6)), [0, 0, 0, 0, 0, 0, 1])


def test_exp_matches_the_reference_se3_exp():
    z = np.load(os.path.join(GOLDEN, "ref_helpers.npz"))
    for tau, ref in zip(z["se3_in"], z["se3_out"]):
        np.testing.assert_allclose(lr.matrix(lr.exp(tau.astype(np.float64))), ref, rtol=0, atol=1e-12)


def test_log_inverts_exp():
    xi = _tangents(2)
    X = lr.exp(xi)
    assert np.abs(lr.log(X) - xi).max() <= 1e-12
    Xn = X.copy()
    Xn[:, 3:] *= -1  # either quaternion sign
    assert np.abs(lr.log(Xn) - xi).max() <= 1e-12
    np.testing.assert_array_equal(lr.log(lr.identity(3)), np.zeros((3, 6)))


def test_product_and_inverse():
    a, b = _elements(3), _elements(4)
    assert np.abs(lr.matrix(lr.mul(a, b)) - lr.matrix(a) @ lr.matrix(b)).max() <= 1e-12
    assert np.abs(lr.mul(a, lr.inv(a)) - lr.identity(len(a))).max() <= 1e-12
    assert np.abs(lr.matrix(lr.inv(a)) - np.linalg.inv(lr.matrix(a))).max() <= 1e-12
    np.testing.assert_array_equal(lr.mul(a, lr.identity(len(a))), a)


def test_action_is_the_matrix_action():
    rng = np.random.default_rng(5)
    X = _elements(6)
    p = rng.normal(size=(len(X), 4))
    M = lr.matrix(X)
    assert np.abs(lr.act(X, p) - np.einsum("nij,nj->ni", M, p)).max() <= 1e-12
    ph = np.concatenate([p[:, :3], np.ones((len(X), 1))], -1)
    assert np.abs(lr.act(X, p[:, :3]) - np.einsum("nij,nj->ni", M, ph)[:, :3]).max() <= 1e-12


def test_adjoint_against_central_differences():
    rng = np.random.default_rng(7)
    X = _elements(8)
    a = rng.normal(size=(len(X), 6))
    eps = 1e-5

    def f(s):
        return lr.log(lr.mul(lr.mul(X, lr.exp(s * a)), lr.inv(X)))

    fd = (f(eps) - f(-eps)) / (2 * eps)
    assert np.abs(lr.adj(X, a) - fd).max() <= 1e-8
    # adjT is the transpose: <adjT(b), a> = <b, adj(a)>
    b = rng.normal(size=(len(X), 6))
    assert np.abs((lr.adjT(X, b) * a).sum(-1) - (b * lr.adj(X, a)).sum(-1)).max() <= 1e-12
    # retr is the left perturbation
    assert np.abs(lr.retr(X, a) - lr.mul(lr.exp(a), X)).max() == 0


def _small_case():
    inp = lr.make_reproject_inputs()
    sel = np.array([1, 7, 9, 16, 23, 30, 34])  # (0,1) (1,1) (1,3) (2,4) (3,5) (5,0) (5,4)
    inp["ii"], inp["jj"] = inp["ii"][sel], inp["jj"][sel]
    return inp


def test_reprojection_jacobians_against_central_differences():
    inp = _small_case()
    ref = lr.reproject(**inp, jacobian=True)
    ii, jj = inp["ii"], inp["jj"]
    # only where neither branch moves under the perturbation
    ok = ~lr.borderline(ref, rel=1e-3) & (ref["Z1"] > 0.5 * lr.MIN_DEPTH)
    assert ok.mean() > 0.9
    eps = 1e-6
    scale = np.maximum(1.0, np.abs(ref["Jj"]).max())

    def coords_with(poses=None, disps=None):
        q = dict(inp)
        if poses is not None:
            q["poses"] = poses
        if disps is not None:
            q["disps"] = disps
        return lr.reproject(**q)["coords"]

    for name, frames in (("Ji", ii), ("Jj", jj)):
        for k in range(6):
            a = np.zeros(6)
            a[k] = eps
            # one edge at a time: perturbing a frame moves every edge that uses it
            for e in range(len(ii)):
                if ii[e] == jj[e]:
                    continue  # the stereo transform does not depend on the poses
                P, M = inp["poses"].copy(), inp["poses"].copy()
                P[frames[e]] = lr.retr(P[frames[e]], a)
                M[frames[e]] = lr.retr(M[frames[e]], -a)
                fd = (coords_with(poses=P)[e] - coords_with(poses=M)[e]) / (2 * eps)
                err = np.abs(fd - ref[name][e][..., k])[ok[e]].max()
                assert err <= 1e-7 * scale, (name, k, e, err)
    dP, dM = inp["disps"] + eps, inp["disps"] - eps
    fd = (coords_with(disps=dP) - coords_with(disps=dM)) / (2 * eps)
    assert np.abs(fd - ref["Jz"][..., 0])[ok].max() <= 1e-7 * scale
    # the stereo edge's pose Jacobians are still the formulas' (the reference computes them)
    assert np.isfinite(ref["Ji"]).all() and np.isfinite(ref["Jj"]).all()


def test_reproject_inputs_cover_both_branches():
    inp = lr.make_reproject_inputs()
    assert inp["disps"].shape == (6, 30, 41) and len(inp["ii"]) == 36
    ref = lr.reproject(**inp)
    v = ref["valid"]
    assert v.size == 44280
    assert abs(v.mean() - 0.944) < 5e-3 and 0 < (v == 0).sum()
    assert (ref["Z1"] < 0.5 * lr.MIN_DEPTH).any()
    assert not lr.borderline(ref, rel=1e-5).any()
    # the same after the inputs are rounded to float32 (what the GPU tests feed)
    r32 = lr.reproject(**{k: (a.astype(np.float32).astype(np.float64) if a.dtype == np.float64 else a)
                          for k, a in inp.items()})
    assert not lr.borderline(r32, rel=1e-5).any()
    np.testing.assert_array_equal(r32["valid"], v)


def test_fp32_evaluation_stays_in_fp32():
    inp = {k: (a.astype(np.float32) if a.dtype == np.float64 else a) for k, a in lr.make_reproject_inputs().items()}
    out = lr.reproject(**inp, jacobian=True, return_depth=True)
    for k, a in out.items():
        assert a.dtype == np.float32, k
    xi = _tangents().astype(np.float32)
    X = lr.exp(xi)
    for a in (X, lr.log(X), lr.inv(X), lr.mul(X, X), lr.matrix(X), lr.adj(X, xi), lr.adjT(X, xi), lr.retr(X, xi),
              lr.act(X, xi[:, :3]), lr.act(X, xi[:, :4])):
        assert a.dtype == np.float32


@pytest.mark.parametrize("return_depth", [False, True])
def test_reprojection_matches_the_reference_composition(return_depth):
    """tests/golden/ref_reproject.npz: the reference's projective_transform
    over the oracle's group algebra (make_reproject_fixtures.py)."""
    z = np.load(os.path.join(GOLDEN, "ref_reproject.npz"))
    ref = lr.reproject(z["poses"], z["disps"], z["intrinsics"], z["ii"], z["jj"], jacobian=True,
                       return_depth=return_depth)
    tag = "d1" if return_depth else "d0"
    assert (z["ii"] == z["jj"]).sum() == 1
    for name in ("coords", "valid", "Ji", "Jj", "Jz"):
        want = z[f"{tag}_{name}"][0]
        assert want.shape == ref[name].shape, name
        assert np.abs(ref[name] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name
