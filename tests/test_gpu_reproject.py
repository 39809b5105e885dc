"""GPU tests of the fused reprojection (csrc/lie.hip k_reproject,
wgsr.frontend.reproject) and of the same steps composed through the
``lietorch`` drop-in, on tests/_lie_ref.make_reproject_inputs() (6 frames, 30 x
41, all 36 ordered pairs) and on the inputs of tests/golden/ref_reproject.npz
(the reference's projective_transform, 4 frames, 12 x 17, 8 edges).

Checked against the float64 oracle (tests/_lie_ref.reproject) and, on the
fixture's inputs, against the recorded outputs of the reference's own code.

Tolerance (derived, never fitted to the kernel): the oracle's formulas are
evaluated once in fp32 numpy on the CPU; per output its worst error against
float64 over the test's own pixels, relative to the oracle's per-element
magnitude (the same expression on absolute values), is measured, and the GPU's
bound is 4 x that (FMA contraction; the device's division and reciprocal
against numpy's), with a floor of 2^-22 x magnitude.  An element whose
magnitude is 0 (the structural zeros of the Jacobians) must be exactly 0.
``valid`` must be exact outside borderline pixels (depth within 1e-5 x
magnitude of 0.2 or 0.1), which may be at most 1 % of all.  Each test prints
the worst observed ratio of GPU error to bound.
"""
import os

import numpy as np
import pytest
import torch

import _lie_ref as lr
from _util import GOLDEN

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22
NAMES = ("coords", "valid", "Ji", "Jj", "Jz")
_cache = {}


def _case(which):
    """inputs (float32), the float64 oracle and the derived relative bounds,
    computed once per input set and shared"""
    if which in _cache:
        return _cache[which]
    if which == "main":
        inp = lr.make_reproject_inputs()
        recorded = None
    else:
        z = np.load(os.path.join(GOLDEN, "ref_reproject.npz"))
        inp = {k: z[k] for k in ("poses", "disps", "intrinsics", "ii", "jj")}
        recorded = {d: {n: z[f"d{int(d)}_{n}"][0] for n in NAMES} for d in (False, True)}
    in32 = {k: (a.astype(np.float32) if a.dtype == np.float64 else a) for k, a in inp.items()}
    in64 = {k: (a.astype(np.float64) if a.dtype == np.float32 else a) for k, a in in32.items()}
    if recorded is not None:  # the fixture's inputs are float32 values
        for k in in64:
            np.testing.assert_array_equal(in64[k], inp[k])
    ref, bound = {}, {}
    for depth in (False, True):
        r = lr.reproject(**in64, jacobian=True, return_depth=depth)
        f = lr.reproject(**in32, jacobian=True, return_depth=depth)
        edge = lr.borderline(r)
        keep = ~edge
        b = {}
        for n in ("coords", "Ji", "Jj", "Jz"):
            m = r[n + "_mag"]
            err = np.abs(f[n].astype(np.float64) - r[n])
            nz = (m > 0) & keep.reshape(keep.shape + (1,) * (m.ndim - keep.ndim))
            assert (err[m == 0] == 0).all(), n
            b[n] = max(4 * float((err[nz] / m[nz]).max()), FLOOR)
        ref[depth], bound[depth] = r, b
        if recorded is not None:  # the oracle is the reference's composition (also tests/test_lie_ref.py)
            for n in NAMES:
                assert np.abs(r[n] - recorded[depth][n]).max() <= 1e-12 * max(1.0, np.abs(r[n]).max()), n
    dev = {k: torch.from_numpy(a).cuda() for k, a in in32.items()}
    _cache[which] = (dev, ref, bound, recorded)
    return _cache[which]


def _compare(tag, got, r, b, worst):
    """got: dict name -> device tensor [1, E, ...]; r: the oracle's outputs"""
    edge = lr.borderline(r)
    assert edge.mean() <= 0.01, (tag, edge.mean())
    v = r["valid"][~edge]
    assert (v == 1).any() and (v == 0).any(), tag
    for n, t in got.items():
        a = t.detach().cpu().numpy().astype(np.float64)
        assert a.shape == (1,) + r[n].shape, (tag, n, a.shape, r[n].shape)
        a = a[0]
        assert np.isfinite(a).all(), (tag, n)
        keep = ~edge.reshape(edge.shape + (1,) * (a.ndim - edge.ndim))
        keep = np.broadcast_to(keep, a.shape)
        if n == "valid":
            assert set(np.unique(a)) <= {0.0, 1.0}
            np.testing.assert_array_equal(a[keep], r[n][keep], err_msg=f"{tag} valid")
            continue
        m = r[n + "_mag"]
        err = np.abs(a - r[n])
        assert (err[(m == 0) & keep] == 0).all(), (tag, n, "structural zeros")
        nz = (m > 0) & keep
        ratio = float((err[nz] / (b[n] * m[nz])).max())
        worst[n] = max(worst.get(n, 0.0), ratio)
        assert ratio <= 1.0, (tag, n, ratio, b[n])


def _bounds_line(b):
    return ", ".join(f"{n} {v:.3g}" for n, v in b.items())


@pytest.mark.parametrize("return_depth", [False, True])
@pytest.mark.parametrize("jacobian", [False, True])
@pytest.mark.parametrize("which", ["main", "fixture"])
def test_fused_kernel(which, jacobian, return_depth):
    from wgsr import frontend
    dev, ref, bound, _ = _case(which)
    out = frontend.reproject(dev["poses"], dev["disps"], dev["intrinsics"], dev["ii"], dev["jj"], jacobian=jacobian,
                             return_depth=return_depth)
    got = {"coords": out[0], "valid": out[1]}
    if jacobian:
        assert len(out) == 3
        got.update(zip(("Ji", "Jj", "Jz"), out[2]))
    else:
        assert len(out) == 2
    assert got["coords"].shape[-1] == (3 if return_depth else 2)
    worst = {}
    _compare(f"fused {which}", got, ref[return_depth], bound[return_depth], worst)
    print(f"\nfused {which} jacobian={jacobian} depth={return_depth}: relative bounds {_bounds_line(bound[return_depth])}"
          f"; worst GPU error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _composed(poses, disps, intrinsics, ii, jj, return_depth):
    """the steps of section 2, one group operation or torch expression each"""
    from lietorch import SE3
    ht, wd = disps.shape[1:]
    dev = poses.device
    G = SE3(poses[None])
    Gij = G[:, jj] * G[:, ii].inv()
    Gij.data[:, ii == jj] = torch.tensor(lr.STEREO, device=dev)
    Ki, Kj = intrinsics[ii][None, :, None, None], intrinsics[jj][None, :, None, None]
    v, u = torch.meshgrid(torch.arange(ht, device=dev).float(), torch.arange(wd, device=dev).float(), indexing="ij")
    d = disps[ii][None]
    one = torch.ones_like(d)
    X0 = torch.stack([(u - Ki[..., 2]) / Ki[..., 0], (v - Ki[..., 3]) / Ki[..., 1], one, d], dim=-1)
    X1 = Gij[:, :, None, None] * X0
    X, Y, Z, D = X1.unbind(-1)
    fx, fy, cx, cy = Kj.unbind(-1)
    iz = 1.0 / torch.where(Z < 0.5 * lr.MIN_DEPTH, one, Z)
    cs = [fx * (X * iz) + cx, fy * (Y * iz) + cy] + ([D * iz] if return_depth else [])
    valid = ((Z > lr.MIN_DEPTH) & (X0[..., 2] > lr.MIN_DEPTH)).float()[..., None]
    o = torch.zeros_like(d)
    Jp = torch.stack([fx * iz, o, -fx * X * iz * iz, o, o, fy * iz, -fy * Y * iz * iz, o], -1).view(d.shape + (2, 4))
    Ja = torch.stack([D, o, o, o, Z, -Y, o, D, o, -Z, o, X, o, o, D, Y, -X, o, o, o, o, o, o, o],
                     -1).view(d.shape + (4, 6))
    Jj = Jp @ Ja
    Ji = -Gij[:, :, None, None, None].adjT(Jj)
    e4 = torch.zeros_like(X0)
    e4[..., 3] = 1.0
    Jz = Jp @ (Gij[:, :, None, None] * e4)[..., None]
    return {"coords": torch.stack(cs, -1), "valid": valid, "Ji": Ji, "Jj": Jj, "Jz": Jz}


@pytest.mark.parametrize("which", ["main", "fixture"])
def test_composition_through_the_drop_in(which):
    dev, ref, bound, _ = _case(which)
    worst = {}
    with torch.no_grad():
        for depth in (False, True):
            got = _composed(dev["poses"], dev["disps"], dev["intrinsics"], dev["ii"], dev["jj"], depth)
            _compare(f"composed {which}", got, ref[depth], bound[depth], worst)
    print(f"\ncomposed {which}: worst GPU error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_unchecked_call_captures_into_a_graph():
    """check=False makes no host read: the call is captured, and the replay
    gives the eager result bit for bit"""
    from wgsr import frontend
    dev, _, _, _ = _case("fixture")
    args = (dev["poses"], dev["disps"], dev["intrinsics"], dev["ii"], dev["jj"])
    c0, v0, J0 = frontend.reproject(*args, jacobian=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c1, v1, J1 = frontend.reproject(*args, jacobian=True, check=False)
    for t in (c1, v1) + J1:
        t.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip((c0, v0) + J0, (c1, v1) + J1):
        assert torch.equal(a, b)


def test_shared_intrinsics_and_edge_cases():
    from wgsr import frontend
    dev, ref, bound, _ = _case("main")
    # one [4] intrinsics vector = every frame's row equal to it
    K = dev["intrinsics"][2].contiguous()
    a = frontend.reproject(dev["poses"], dev["disps"], K, dev["ii"], dev["jj"], jacobian=True)
    b = frontend.reproject(dev["poses"], dev["disps"], K[None].repeat(6, 1), dev["ii"], dev["jj"], jacobian=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
    # an empty edge list: empty tensors of the reference's shapes
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    c, v, (Ji, Jj, Jz) = frontend.reproject(dev["poses"], dev["disps"], dev["intrinsics"], e, e, jacobian=True,
                                            return_depth=True)
    assert c.shape == (1, 0, 30, 41, 3) and v.shape == (1, 0, 30, 41, 1)
    assert Ji.shape == Jj.shape == (1, 0, 30, 41, 2, 6) and Jz.shape == (1, 0, 30, 41, 2, 1)
    # an index outside the frames: refused on the host; with check=False the edge reads nothing (NaN)
    bad = torch.tensor([0, 6], dtype=torch.int64, device="cuda")
    ok = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="must index frames"):
        frontend.reproject(dev["poses"], dev["disps"], dev["intrinsics"], bad, ok)
    c, v = frontend.reproject(dev["poses"], dev["disps"], dev["intrinsics"], bad, ok, check=False)
    assert torch.isfinite(c[0, 0]).all() and torch.isnan(c[0, 1]).all() and torch.isnan(v[0, 1]).all()
    with pytest.raises(RuntimeError, match="int64"):
        frontend.reproject(dev["poses"], dev["disps"], dev["intrinsics"], ok.int(), ok)
    with pytest.raises(RuntimeError, match="float32"):
        frontend.reproject(dev["poses"].double(), dev["disps"], dev["intrinsics"], ok, ok)
