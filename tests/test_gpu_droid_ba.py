"""GPU tests of ``droid_backends.ba`` (csrc/droid_ba.hip) against the numpy
oracle of tests/_droid_ba_ref.py.

Tolerances are derived, not fixed: a quantity may deviate from the float64
oracle by 8 x max|oracle(float32) - oracle(float64)| on that case, plus 1e-6 x
max|quantity| (H: per 6 x 6 block, relative to the block's largest entry).
The factor 8 covers another summation order over about 10^3 pixels; every
test prints its measured ratio (DESIGN.md section 4 records the worst).
tests/test_droid_ba_ref.py shows the cases to be decisive: no pixel near the
depth cut, a successful factorisation, and a step at least 100 x the spread.

Case b's extra edges: a stereo edge (2, 2) and the edge (3, far frame), every
pixel of which falls under the depth cut in the far frame.
"""
import functools

import numpy as np
import pytest
import torch

import _droid_ba_ref as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ARGS = ("poses", "disps", "intr", "disps_sens", "targets", "weights", "eta", "ii", "jj")


def tensors(c):
    return [torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ARGS]


@functools.lru_cache(maxsize=None)
def oracle(name, iterations, lm=1e-4, ep=0.1, motion_only=False, depth_only=False):
    """(float64 result, float32 result), computed once per configuration."""
    c = B.case(name)
    kw = dict(motion_only=motion_only, depth_only=depth_only)
    return (B.run(c, iterations, lm, ep, dtype=np.float64, **kw), B.run(c, iterations, lm, ep, dtype=np.float32, **kw))


def close(what, got, o64, o32):
    """Assert the derived bound and return the measured ratio err / spread."""
    got, o64, o32 = (np.asarray(a, np.float64) for a in (got, o64, o32))
    assert got.shape == o64.shape, (what, got.shape, o64.shape)
    err, spread, scale = np.abs(got - o64).max(), np.abs(o32 - o64).max(), np.abs(o64).max()
    ratio = err / spread if spread > 0 else (0.0 if err == 0 else np.inf)
    print(f"{what}: err {err:.3e} spread {spread:.3e} ratio {ratio:.2f} (scale {scale:.3e})")
    assert err <= 8 * spread + 1e-6 * scale, what
    return ratio


def close_blocks(what, got, o64, o32):
    got, o64, o32 = (np.asarray(a, np.float64) for a in (got, o64, o32))
    P = o64.shape[0] // 6
    blk = lambda M: np.abs(M).reshape(P, 6, P, 6).max((1, 3))  # noqa: E731
    err, spread, scale = blk(got - o64), blk(o32 - o64), blk(o64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(spread > 0, err / spread, np.where(err == 0, 0.0, np.inf))
    print(f"{what}: worst block ratio {ratio.max():.2f} (err {err.max():.3e}, spread {spread.max():.3e})")
    assert (err <= 8 * spread + 1e-6 * scale).all(), what
    return ratio.max()


# ---------------------------------------------------------------------------
# the system of one linearisation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_system_matches_the_oracle(name):
    import droid_backends
    c = B.case(name)
    o64, o32 = (r["first"] for r in oracle(name, 1))
    args = tensors(c)
    before = [args[0].clone(), args[1].clone()]
    H, g, C, w, dx = droid_backends._ba_system(*args, c["t0"], c["t1"], 1e-4, 0.1)
    assert H.dtype == g.dtype == torch.float64 and C.dtype == w.dtype == dx.dtype == torch.float32
    assert torch.equal(args[0], before[0]) and torch.equal(args[1], before[1])
    close_blocks("H", H.cpu().numpy(), o64["H"], o32["H"])
    close("g", g.cpu().numpy(), o64["g"], o32["g"])
    close("C", C.cpu().numpy(), o64["C"], o32["C"])
    close("w", w.cpu().numpy(), o64["w"], o32["w"])
    close("dx", dx.cpu().numpy(), o64["dx"], o32["dx"])
    assert np.array_equal(H.cpu().numpy(), H.cpu().numpy().T)


def test_system_motion_only_is_the_pose_block():
    import droid_backends
    c = B.case("a")
    o64, o32 = (r["first"] for r in oracle("a", 1, motion_only=True))
    H, g, C, w, dx = droid_backends._ba_system(*tensors(c), c["t0"], c["t1"], 1e-4, 0.1, motion_only=True)
    assert C is None and w is None
    close_blocks("H", H.cpu().numpy(), o64["H"], o32["H"])
    close("g", g.cpu().numpy(), o64["g"], o32["g"])
    close("dx", dx.cpu().numpy(), o64["dx"], o32["dx"])


# ---------------------------------------------------------------------------
# the full op
# ---------------------------------------------------------------------------
FULL = [("a", {}), ("a", dict(motion_only=True)), ("a", dict(depth_only=True)), ("a", dict(lm=1e-5, ep=1e-2)),
        ("a_sens", {}), ("b", {}), ("c", {}),
        # the solver's two paths: 6 P = 90 is past the LDS limit (84); 6 P = 180 has several tiles in the
        # blocked path's trailing update; and the smallest system
        ("band15", {}), ("band30", {}), ("band14", {}), ("band1", {})]


def run_gpu(name, iterations=2, lm=1e-4, ep=0.1, motion_only=False, depth_only=False, **kw):
    import droid_backends
    c = B.case(name)
    args = tensors(c)
    dx, dz = droid_backends.ba(*args, c["t0"], c["t1"], iterations, lm, ep, motion_only, depth_only, **kw)
    return args[0], args[1], dx, dz


@pytest.mark.parametrize("name,kw", FULL, ids=[f"{n}-{'-'.join(k) or 'full'}" for n, k in FULL])
def test_ba_matches_the_oracle(name, kw):
    c = B.case(name)
    o64, o32 = oracle(name, 2, **kw)
    assert o64["chol_ok"] and not o64["near"]
    poses, disps, dx, dz = run_gpu(name, **kw)
    close("poses", poses.cpu().numpy(), o64["poses"], o32["poses"])
    close("disps", disps.cpu().numpy(), o64["disps"], o32["disps"])
    close("dx", dx.cpu().numpy(), o64["dx"], o32["dx"])
    if kw.get("motion_only"):
        assert dz.numel() == 0
        assert torch.equal(disps.cpu(), torch.from_numpy(c["disps"]))
    else:
        close("dz", dz.cpu().numpy(), o64["dz"], o32["dz"])
    if kw.get("depth_only"):
        assert torch.equal(poses.cpu(), torch.from_numpy(c["poses"]))
    # fixed poses never move
    assert torch.equal(poses[:c["t0"]].cpu(), torch.from_numpy(c["poses"][:c["t0"]]))


def test_rank_deficient_system_gives_a_zero_step():
    """ep = lm = 0 and all weights zero: the pose block is the zero matrix,
    the first pivot fails, dx = 0 and the poses keep their bits."""
    import droid_backends
    c = dict(B.case("a"))
    c["weights"] = np.zeros_like(c["weights"])
    args = tensors(c)
    dx, dz = droid_backends.ba(*args, c["t0"], c["t1"], 2, 0.0, 0.0, True, False)
    assert (dx == 0).all() and dz.numel() == 0
    assert torch.equal(args[0].cpu(), torch.from_numpy(c["poses"]))


@pytest.mark.parametrize("what", ["eta_rows", "ii_is_num", "jj_is_t1"])
def test_status_word_leaves_the_state_untouched(what):
    """Bounds checks on the device: the bad index is never dereferenced."""
    import droid_backends
    c = dict(B.case("a"))
    num = len(c["poses"])
    if what == "eta_rows":
        c["eta"] = np.ascontiguousarray(np.concatenate([c["eta"], c["eta"][:1]]))   # one row too many
        match = "eta's rows"
    elif what == "ii_is_num":
        c["ii"] = c["ii"].copy()
        c["ii"][3] = num
        match = r"outside \[0, num\)"
    else:
        c["t1"] = c["t1"] - 1     # (kx is unchanged: frame 4 is a source)
        match = "jj entry is >= t1"
    args = tensors(c)
    with pytest.raises(RuntimeError, match=match):
        droid_backends.ba(*args, c["t0"], c["t1"], 2, 1e-4, 0.1, False, False)
    assert torch.equal(args[0].cpu(), torch.from_numpy(c["poses"]))
    assert torch.equal(args[1].cpu(), torch.from_numpy(c["disps"]))


def test_eta_with_a_row_too_few_is_refused():
    import droid_backends
    c = dict(B.case("c"))     # K = 5 > P = 3: one row fewer still passes the host's size checks
    c["eta"] = np.ascontiguousarray(c["eta"][:-1])
    args = tensors(c)
    with pytest.raises(RuntimeError, match="eta's rows"):
        droid_backends.ba(*args, c["t0"], c["t1"], 2, 1e-4, 0.1, False, False)
    assert torch.equal(args[0].cpu(), torch.from_numpy(c["poses"]))
    assert torch.equal(args[1].cpu(), torch.from_numpy(c["disps"]))


@pytest.mark.parametrize("name", ["b", "band15"])
def test_two_runs_are_bit_identical(name):
    first = [t.cpu() for t in run_gpu(name)]
    second = [t.cpu() for t in run_gpu(name)]
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_unchecked_call_captures_into_a_graph():
    """check=False makes no synchronisation: the call is captured and the
    replay gives the eager result bit for bit."""
    import droid_backends
    c = B.case("a")
    eager = [t.clone() for t in run_gpu("a")]
    args = tensors(c)
    poses0, disps0 = args[0].clone(), args[1].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dx, dz = droid_backends.ba(*args, c["t0"], c["t1"], 2, 1e-4, 0.1, False, False, check=False)
    for _ in range(2):   # a replay starts from the state it is given
        args[0].copy_(poses0)
        args[1].copy_(disps0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, (args[0], args[1], dx, dz)):
            assert torch.equal(a, b)


def test_frontend_ba_is_the_composition_of_its_parts():
    import droid_backends
    from wgsr import frontend
    c = B.case("a_sens")
    poses, disps, intr, sens, targets, weights, eta, ii, jj = tensors(c)
    N, (ht, wd) = len(c["ii"]), disps.shape[1:]
    # the update operator's layout [1, N, ht, wd, 2]
    target5 = targets.permute(0, 2, 3, 1).contiguous()[None]
    weight5 = weights.permute(0, 2, 3, 1).contiguous()[None]
    unc = torch.linspace(0.5, 1.0, disps.numel(), device=DEV).reshape(disps.shape)
    mask = sens > 0
    mono = torch.where(mask, sens, torch.full_like(sens, 0.3))
    p1, d1 = poses.clone(), disps.clone()
    out1 = frontend.ba(p1, d1, intr, target5, weight5, eta, ii, jj, t0=1, t1=None, iters=2,
                       uncertainties_inv=unc, mono_disps=mono, mono_valid_mask=mask)
    p2, d2 = poses.clone(), disps.clone()
    w2 = (weight5 * unc[ii][None, :, :, :, None]).view(N, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    out2 = droid_backends.ba(p2, d2, intr, (mono * mask).contiguous(), targets, w2, eta, ii, jj, 1, c["t1"], 2, 1e-4,
                             0.1, False, False)
    d2.clamp_(min=1e-5)
    assert torch.equal(p1, p2) and torch.equal(d1, d2)
    assert torch.equal(out1[0], out2[0]) and torch.equal(out1[1], out2[1])
    assert not torch.equal(p1, poses) and not torch.equal(d1, disps)
    # without sensor disparities: zeros
    p3, d3 = poses.clone(), disps.clone()
    frontend.ba(p3, d3, intr, target5, weight5, eta, ii, jj, motion_only=True)
    p4, d4 = poses.clone(), disps.clone()
    droid_backends.ba(p4, d4, intr, torch.zeros_like(disps), targets, weights, eta, ii, jj, 1, c["t1"], 2, 1e-4, 0.1,
                      True, False)
    assert torch.equal(p3, p4) and torch.equal(d3, d4.clamp(min=1e-5))
