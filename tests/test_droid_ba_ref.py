"""CPU tests of ``droid_backends.ba`` (no GPU needed): the numpy oracle
(tests/_droid_ba_ref.py) against independent statements of the same
operation, the conditions that make the GPU tests
(tests/test_gpu_droid_ba.py) decisive, and the module surface."""
import numpy as np
import pytest
import torch

import _droid_ba_ref as B

# (case, kwargs of the op) of every GPU comparison with the oracle
DECISIVE = [("a", {}), ("b", {}), ("c", {}), ("a", dict(motion_only=True)), ("a", dict(depth_only=True)),
            ("a", dict(lm=1e-5, ep=1e-2)), ("a_sens", {}), ("band15", {}), ("band30", {}),
            ("band14", {}), ("band1", {})]


def test_jacobians_match_central_differences():
    c = B.case("a")
    poses, disps, intr = (c[k].astype(np.float64) for k in ("poses", "disps", "intr"))
    i, j, eps = 2, 3, 1e-6
    Ji, Jj, Jz, _, valid, z = B.jacobians(poses[i], poses[j], disps[i], intr, np.float64)
    assert valid.all() and np.abs(z - B.MIN_DEPTH).min() > 1e-3

    def proj(pi, pj, d):
        return B.project(pi, pj, d, intr, np.float64)[0]

    worst = 0.0
    for n in range(6):
        xi = np.zeros(6)
        xi[n] = eps
        fd_j = (proj(poses[i], B.retract(poses[j], xi, np.float64), disps[i])
                - proj(poses[i], B.retract(poses[j], -xi, np.float64), disps[i])) / (2 * eps)
        fd_i = (proj(B.retract(poses[i], xi, np.float64), poses[j], disps[i])
                - proj(B.retract(poses[i], -xi, np.float64), poses[j], disps[i])) / (2 * eps)
        worst = max(worst, np.abs(fd_j - Jj[:, n]).max(), np.abs(fd_i - Ji[:, n]).max())
    fd_z = (proj(poses[i], poses[j], disps[i] + eps) - proj(poses[i], poses[j], disps[i] - eps)) / (2 * eps)
    worst = max(worst, np.abs(fd_z - Jz).max())
    scale = max(np.abs(Jj).max(), np.abs(Ji).max())
    print("worst |J - central difference|", worst, "of", scale)
    assert worst <= 1e-7 * scale


def test_schur_elimination_matches_the_full_dense_solve():
    """3 frames, 6 x 8: the eliminated solve (oracle, quirk off) against the
    full damped normal equations over poses and disparities, built densely
    from the per-edge terms."""
    c = B.case("small")
    lm, ep = float(np.float32(1e-4)), float(np.float32(0.1))   # (the op takes them as float32)
    out = B.run(c, 1, lm, ep, quirk=False)
    first = out["first"]
    ii, jj, t0, t1 = list(c["ii"]), list(c["jj"]), c["t0"], c["t1"]
    P, kx, HW = t1 - t0, first["kx"], 48
    K = len(kx)
    n = 6 * P
    M, rhs = np.zeros((n + K * HW, n + K * HW)), np.zeros(n + K * HW)
    for e, ed in enumerate(first["edges"]):
        k = kx.index(ii[e])
        cols = slice(n + k * HW, n + (k + 1) * HW)
        ends = (ii[e] - t0, jj[e] - t0)
        for x, fx in enumerate(ends):
            if not 0 <= fx < P:
                continue
            rhs[6 * fx:6 * fx + 6] += ed["v"][6 * x:6 * x + 6]
            Ex = ed["Ei"] if x == 0 else ed["Ej"]
            M[6 * fx:6 * fx + 6, cols] += Ex
            M[cols, 6 * fx:6 * fx + 6] += Ex.T
            for y, fy in enumerate(ends):
                if 0 <= fy < P:
                    M[6 * fx:6 * fx + 6, 6 * fy:6 * fy + 6] += ed["H"][6 * x:6 * x + 6, 6 * y:6 * y + 6]
    Cd = first["C"].reshape(-1).astype(np.float64)
    M[np.arange(n, n + K * HW), np.arange(n, n + K * HW)] = Cd
    rhs[n:] = first["w"].reshape(-1)
    # the damping acts on the reduced system's diagonal
    E = M[:n, n:]
    red = M[:n, :n] - (E / Cd) @ E.T
    M[np.arange(n), np.arange(n)] += ep + lm * np.diag(red)
    # (solved after symmetric diagonal scaling, with one refinement step: the
    # diagonal spans seven orders of magnitude)
    sc = 1 / np.sqrt(np.diag(M))
    Ms = M * sc[:, None] * sc[None, :]
    full = np.linalg.solve(Ms, rhs * sc)
    full += np.linalg.solve(Ms, rhs * sc - Ms @ full)
    full *= sc
    dx, dz = full[:n].reshape(P, 6), full[n:].reshape(K, HW)
    ex, ez = np.abs(dx - first["dx"]).max() / np.abs(dx).max(), np.abs(dz - first["dz"]).max() / np.abs(dz).max()
    print("eliminated vs full: dx", ex, "dz", ez)
    assert ex <= 1e-9 and ez <= 1e-9
    # with the quirk, only the term of pose t0's own step differs
    quirk = B.run(c, 1, lm, ep)["first"]
    assert np.array_equal(quirk["dx"], first["dx"])
    assert np.abs(quirk["dz"] - first["dz"]).max() > 1e-6 * np.abs(dz).max()


@pytest.mark.parametrize("name,kw", DECISIVE, ids=[f"{n}-{'-'.join(k) or 'full'}" for n, k in DECISIVE])
def test_gpu_cases_are_decisive(name, kw):
    c = B.case(name)
    r64 = B.run(c, 2, dtype=np.float64, **kw)
    r32 = B.run(c, 2, dtype=np.float32, **kw)
    assert not r64["near"] and not r32["near"]
    assert r64["chol_ok"] and r32["chol_ok"]
    dx64, dx32 = r64["first"]["dx"], r32["first"]["dx"].astype(np.float64)
    spread, norm = np.abs(dx64 - dx32).max(), np.linalg.norm(dx64)
    print("first dx norm", norm, "float32 / float64 spread", spread, "ratio", norm / spread)
    assert norm >= 100 * spread
    assert spread <= 1e-3 * np.abs(dx64).max()


def test_rank_deficient_system_is_reported():
    c = dict(B.case("a"))
    c["weights"] = np.zeros_like(c["weights"])
    out = B.run(c, 1, 0.0, 0.0, motion_only=True)
    assert not out["chol_ok"] and (out["dx"] == 0).all()
    assert np.array_equal(out["poses"], c["poses"].astype(np.float64))


def _host_args(c):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c.items() if isinstance(v, np.ndarray)}
    return [t["poses"], t["disps"], t["intr"], t["disps_sens"], t["targets"], t["weights"], t["eta"], t["ii"],
            t["jj"], c["t0"], c["t1"], 2, 1e-4, 0.1, False, False]


def test_ba_module_surface():
    import droid_backends
    args = _host_args(B.case("small"))
    # host tensors never reach a kernel
    with pytest.raises(RuntimeError, match="HIP device"):
        droid_backends.ba(*args)
    bad = list(args)
    bad[4] = torch.zeros(6, 2, 8, 6).transpose(2, 3)
    with pytest.raises(RuntimeError, match="targets must be contiguous"):
        droid_backends.ba(*bad)
    # any other call form: the overload is not implemented
    with pytest.raises(NotImplementedError, match="only the reference's call form"):
        droid_backends.ba(*args[:15])
    assert callable(droid_backends._ba_system)
    for name in ("projmap", "altcorr_forward", "altcorr_backward"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(droid_backends, name)()
