"""GPU tests of the SE3 group kernels (csrc/lie.hip) through the ``lietorch``
drop-in, against the float64 oracle tests/_lie_ref.py.

Tolerance (derived, never fitted to the kernel): the same formulas are
evaluated once in fp32 numpy on the CPU; its worst error against the float64
oracle over the test's own inputs, per element relative to the row's magnitude
(the largest absolute value among the row's inputs and its exact result), is
measured, and the GPU's bound is 4 x that (FMA contraction, and the device's
sin / cos / atan2 / sqrt differing from numpy's by a few ulp), with a floor of
2^-22.  Each test prints the worst observed ratio of GPU error to bound.
"""
import numpy as np
import pytest
import torch

import _lie_ref as lr

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22
THETAS = (0.0, 1e-6, 1e-3, 0.1, 0.2499, 0.26, 1.0, 2.0, 3.0)  # exactly 0, the series branch, O(1), 3.0 rad


def _inputs(n, seed):
    """n tangent vectors whose angles cycle through THETAS, n more for the
    second operand, n points; float32"""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    th = np.array([THETAS[k % len(THETAS)] for k in range(n)])[:, None]
    xi = np.concatenate([rng.normal(size=(n, 3)), th * axis], -1).astype(np.float32)
    xi[th[:, 0] == 0] = 0
    a = rng.normal(size=(n, 6)).astype(np.float32)
    p = rng.normal(size=(n, 4)).astype(np.float32)
    return xi, a, p


def _check(name, gpu, args32, fn, worst):
    """gpu: the device result; fn(*args) the oracle's function of the inputs"""
    ref = fn(*[x.astype(np.float64) for x in args32])
    f32 = fn(*args32)
    assert f32.dtype == np.float32
    got = gpu.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    bs = np.broadcast_shapes(*[x.shape[:-1] for x in args32])
    nb = int(np.prod(bs))
    mag = np.abs(ref).reshape(nb, -1).max(-1)
    for x in args32:
        mag = np.maximum(mag, np.broadcast_to(np.abs(x.astype(np.float64)).max(-1), bs).reshape(-1))
    e_np = (np.abs(f32.astype(np.float64) - ref).reshape(nb, -1).max(-1) / mag).max()
    bound = max(4 * e_np, FLOOR)
    e_gpu = (np.abs(got - ref).reshape(nb, -1).max(-1) / mag).max()
    worst[name] = max(worst.get(name, 0.0), e_gpu / bound)
    assert e_gpu <= bound, (name, e_gpu, bound, e_np)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_every_op_against_the_oracle(n):
    from lietorch import SE3
    xi, a, p = _inputs(n, seed=n)
    X32 = lr.exp(xi)
    Y32 = lr.exp(_inputs(n, seed=n + 7)[0][::-1].copy())
    worst = {}
    with torch.no_grad():
        G, H = SE3(_dev(X32)), SE3(_dev(Y32))
        _check("exp", SE3.exp(_dev(xi)).data, (xi,), lr.exp, worst)
        _check("log", G.log(), (X32,), lr.log, worst)
        Xn = X32.copy()
        Xn[:, 3:] *= -1
        _check("log(-q)", SE3(_dev(Xn)).log(), (Xn,), lr.log, worst)
        _check("inv", G.inv().data, (X32,), lr.inv, worst)
        _check("mul", (G * H).data, (X32, Y32), lr.mul, worst)
        _check("act3", G * _dev(p[:, :3]), (X32, p[:, :3].copy()), lr.act, worst)
        _check("act4", G * _dev(p), (X32, p), lr.act, worst)
        _check("matrix", G.matrix(), (X32,), lr.matrix, worst)
        _check("adj", G.adj(_dev(a)), (X32, a), lr.adj, worst)
        _check("adjT", G.adjT(_dev(a)), (X32, a), lr.adjT, worst)
        _check("retr", G.retr(_dev(xi)).data, (X32, xi), lr.retr, worst)
        assert G.matrix().shape == (n, 4, 4)
    print(f"\nn={n}: worst GPU error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_broadcast_pose_over_a_point_map():
    """[1, 5, 1, 1] x [1, 5, 7, 9, 4]: the pose is passed with its repeat count;
    a pattern that is not a trailing broadcast is expanded"""
    from lietorch import SE3
    xi, a, _ = _inputs(5, seed=3)
    X32 = lr.exp(xi)[None]
    rng = np.random.default_rng(4)
    P = rng.normal(size=(1, 5, 7, 9, 4)).astype(np.float32)
    J = rng.normal(size=(1, 5, 7, 9, 2, 6)).astype(np.float32)
    worst = {}
    with torch.no_grad():
        G = SE3(_dev(X32))
        _check("act4", G[:, :, None, None] * _dev(P), (X32[:, :, None, None], P), lr.act, worst)
        _check("act3", G[:, :, None, None] * _dev(P[..., :3].copy()), (X32[:, :, None, None], P[..., :3].copy()),
               lr.act, worst)
        _check("adjT", G[:, :, None, None, None].adjT(_dev(J)), (X32[:, :, None, None, None], J), lr.adjT, worst)
        # poses varying along the last batch dimension only: the expand path
        Xr = lr.exp(_inputs(9, seed=5)[0])[None, None, None]
        _check("act4 (expanded)", SE3(_dev(Xr)) * _dev(P), (Xr, P), lr.act, worst)
        Ya = lr.exp(_inputs(7, seed=6)[0])[None, None, :, None]
        _check("mul (both broadcast)", (G[:, :, None, None] * SE3(_dev(Ya))).data,
               (X32[:, :, None, None], Ya), lr.mul, worst)
    print("\nbroadcast: worst GPU error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_exact_values():
    from lietorch import SE3
    with torch.no_grad():
        e = SE3.exp(torch.zeros(65, 6, device="cuda")).data.cpu()
        assert torch.equal(e, torch.tensor([0.0, 0, 0, 0, 0, 0, 1]).expand(65, 7))
        Id = SE3.Identity(65, device="cuda")
        assert torch.equal(Id.log().cpu(), torch.zeros(65, 6))
        X = _dev(lr.exp(_inputs(65, seed=11)[0]))
        assert torch.equal((SE3(X) * Id).data, X)
        assert torch.equal(SE3(X).retr(torch.zeros(65, 6, device="cuda")).data, X)
        empty = SE3(torch.zeros(0, 7, device="cuda"))
        assert empty.inv().data.shape == (0, 7) and empty.log().shape == (0, 6)


@pytest.mark.parametrize("s", [0.0, 0.5, 1.0])
def test_trajectory_filler_interpolation(s):
    """trajectory_filler.py:66-70: SE3.exp(log(P1 P0^-1) s) P0"""
    from lietorch import SE3
    P0 = lr.exp(_inputs(130, seed=21)[0])
    P1 = lr.exp(_inputs(130, seed=22)[0][::-1].copy())
    sv = np.full((130, 1), s, np.float32)

    def chain(P0, P1, sv):
        return lr.mul(lr.exp(lr.log(lr.mul(P1, lr.inv(P0))) * sv), P0)

    worst = {}
    with torch.no_grad():
        G0, G1 = SE3(_dev(P0)), SE3(_dev(P1))
        dP = G1 * G0.inv()
        Gs = SE3.exp(dP.log() * _dev(sv)) * G0
    _check(f"s={s}", Gs.data, (P0, P1, np.broadcast_to(sv, (130, 1)).copy()), chain, worst)
    ref = chain(P0.astype(np.float64), P1.astype(np.float64), sv.astype(np.float64))
    end = (P0, None, P1)[int(2 * s)]
    if end is not None:  # the end points themselves, up to the quaternion's sign
        q = ref[:, 3:] * np.sign((ref[:, 3:] * end[:, 3:]).sum(-1, keepdims=True))
        assert np.abs(ref[:, :3] - end[:, :3]).max() < 1e-5 and np.abs(q - end[:, 3:]).max() < 1e-5
    print(f"\ntrajectory s={s}: worst GPU error / bound {worst[f's={s}']:.3f}")
