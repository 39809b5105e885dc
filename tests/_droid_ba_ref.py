"""numpy restatement of ``droid_backends.ba`` (csrc/droid_ba.hip), written
from the operation's definition, and the generator of
the cases its tests share.

``dtype`` selects the arithmetic of the per-pixel part (relative pose,
residuals, Jacobians, E, C, w, Q, dz, the retraction): float64, or float32 as
the kernels compute it.  In both modes the cross-pixel sums, the reduced
system and its Cholesky solve (``numpy.linalg.cholesky``) are float64.  The
difference between the two modes is the yardstick of the GPU tests'
tolerances.

Notation: N edges (ii[e], jj[e]); frames [t0, t1) have free poses, P = t1 - t0;
kx = sorted({t0..t1-1} u set(ii)) are the K frames whose disparities are
variables; HW = ht * wd.  Pose updates are left-multiplied: T <- exp(xi) T,
xi = (tau, phi).
"""
import functools

import numpy as np

import _droid_ref as R
from _droid_ref import make_inputs, quat_mul

MIN_DEPTH = R.MIN_DEPTH
NEAR_CUT = 1e-5     # a transformed depth this close to MIN_DEPTH is "near the cut"
ALPHA = 0.05
STEREO_T = (-0.1, 0.0, 0.0)


# ---------------------------------------------------------------------------
# rigid transforms in the working dtype
# ---------------------------------------------------------------------------
def _rot_delta(q, X):
    u, w = q[:3], q[3]
    s = 2 * np.cross(u, X)
    return w * s + np.cross(u, s)


def _rotate(q, X):
    return X + _rot_delta(q, X)


def _conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], q.dtype)


def relative(pose_i, pose_j, dtype):
    pi, pj = np.asarray(pose_i, dtype), np.asarray(pose_j, dtype)
    q = quat_mul(pj[3:], _conj(pi[3:])).astype(dtype)
    return q, pj[:3] - _rotate(q, pi[:3])


def exp_se3(xi, dtype):
    """(dt, dq) of exp(xi), xi = (tau, phi)."""
    xi = np.asarray(xi, dtype)
    tau, phi = xi[:3], xi[3:]
    th2 = phi @ phi
    th = np.sqrt(th2)
    if th2 < 1e-8:
        imag = 0.5 - th2 / 48 + th2 * th2 / 3840
        real = 1 - th2 / 8 + th2 * th2 / 384
    else:
        imag, real = np.sin(th / 2) / th, np.cos(th / 2)
    dq = np.array([imag * phi[0], imag * phi[1], imag * phi[2], real], dtype)
    dt = tau.copy()
    if th > 1e-4:
        c1 = np.cross(phi, tau)
        dt = dt + (1 - np.cos(th)) / th2 * c1 + (th - np.sin(th)) / (th * th2) * np.cross(phi, c1)
    return dt.astype(dtype), dq


def retract(pose, xi, dtype):
    """exp(xi) pose."""
    pose = np.asarray(pose, dtype)
    dt, dq = exp_se3(xi, dtype)
    q = quat_mul(dq, pose[3:]).astype(dtype)
    t = _rotate(dq, pose[:3]) + dt
    return np.concatenate([t, q]).astype(dtype)


# ---------------------------------------------------------------------------
# one edge
# ---------------------------------------------------------------------------
def project(pose_i, pose_j, disp_i, intr, dtype, stereo=False):
    """(proj [2, HW], valid [HW], parts): the projection of frame i's pixels
    into frame j; an invalid pixel (Y_z < MIN_DEPTH) has inverse depth 0."""
    intr = np.asarray(intr, dtype)
    fx, fy, cx, cy = intr
    ht, wd = disp_i.shape
    # the rays as the kernel forms them: (u - cx) / fx in the working dtype
    v, u = np.meshgrid(np.arange(ht, dtype=dtype), np.arange(wd, dtype=dtype), indexing="ij")
    X = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1).reshape(-1, 3).astype(dtype)
    h = np.asarray(disp_i, dtype).reshape(-1)
    if stereo:
        q, t = np.array([0, 0, 0, 1], dtype), np.array(STEREO_T, dtype)
    else:
        q, t = relative(pose_i, pose_j, dtype)
    Y = _rotate(q, X) + h[:, None] * t
    x, y, z = Y[:, 0], Y[:, 1], Y[:, 2]
    valid = z >= MIN_DEPTH
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(valid, 1 / z, 0).astype(dtype)
    proj = np.stack([fx * d * x + cx, fy * d * y + cy])
    return proj, valid, (q, t, x, y, z, d, h)


def jacobians(pose_i, pose_j, disp_i, intr, dtype, stereo=False):
    """(Ji [2, 6, HW], Jj [2, 6, HW], Jz [2, HW], proj, valid, z): the
    derivatives of the projection with respect to the two poses' left
    updates and to the source disparity."""
    fx, fy = np.asarray(intr, dtype)[:2]
    proj, valid, (q, t, x, y, z, d, h) = project(pose_i, pose_j, disp_i, intr, dtype, stereo)
    d2, zero = d * d, np.zeros_like(d)
    Jj = np.stack([
        np.stack([fx * (h * d), zero, fx * (-x * h * d2), fx * (-x * y * d2), fx * (1 + x * x * d2), fx * (-y * d)]),
        np.stack([zero, fy * (h * d), fy * (-y * h * d2), fy * (-1 - y * y * d2), fy * (x * y * d2), fy * (x * d)])])
    Jz = np.stack([fx * (t[0] * d - t[2] * (x * d2)), fy * (t[1] * d - t[2] * (y * d2))])
    # J_i = -Ad(T_ij)^T J_j: (a, b) -> -(R^T a, R^T (b + a x t))
    qi = _conj(q)
    Ji = np.empty_like(Jj)
    for r in range(2):
        a, b = Jj[r, :3].T, Jj[r, 3:].T
        Ji[r, :3] = -_rotate(qi, a).T
        Ji[r, 3:] = -_rotate(qi, b + np.cross(a, t)).T
    return Ji.astype(dtype), Jj.astype(dtype), Jz.astype(dtype), proj, valid, z


def linearise_edge(poses, disps, intr, target, weight, i, j, dtype):
    """Step 1 for one edge: dict of H [12, 12], v [12] (float64; rows 0-5 pose
    i, 6-11 pose j), Ei, Ej [6, HW], C, bz [HW] (dtype), near (bool)."""
    stereo = i == j
    Ji, Jj, Jz, proj, valid, z = jacobians(poses[i], poses[j], disps[i], intr, dtype, stereo)
    tg = np.asarray(target, dtype).reshape(2, -1)
    wt = np.where(valid, dtype(0.001) * np.asarray(weight, dtype).reshape(2, -1), 0).astype(dtype)
    r = tg - proj
    C = (wt * Jz * Jz).sum(0)
    bz = (wt * r * Jz).sum(0)
    wp = np.zeros_like(wt) if stereo else wt
    J = np.concatenate([Ji, Jj], 1)                                # [2, 12, HW]
    wJ = wp[:, None, :] * J
    H = (wJ[:, :, None, :] * J[:, None, :, :]).sum((0, 3), dtype=np.float64)
    v = (wJ * r[:, None, :]).sum((0, 2), dtype=np.float64)
    E = (wJ * Jz[:, None, :]).sum(0)                               # [12, HW]
    return dict(H=H, v=v, Ei=E[:6].astype(dtype), Ej=E[6:].astype(dtype), C=C.astype(dtype), bz=bz.astype(dtype),
                near=bool((np.abs(z - MIN_DEPTH) < NEAR_CUT).any()))


# ---------------------------------------------------------------------------
# the op
# ---------------------------------------------------------------------------
def slots(ii, t0, t1):
    return sorted(set(range(t0, t1)) | set(int(i) for i in ii))


def couplings(edges, ii, jj, kx, t0, t1):
    """Per slot k: the list of (pose index relative to t0, E [6, HW]) of the
    frame's couplings to free poses: its own pose through Ei[k] = the sum of
    its edges' E_i, and pose jj[e] through E_j[e]."""
    P = t1 - t0
    out = []
    for f in kx:
        mine = [e for e in range(len(ii)) if ii[e] == f]
        cs = []
        if t0 <= f < t1:
            Ei = np.zeros_like(edges[0]["Ei"])
            for e in mine:
                Ei = Ei + edges[e]["Ei"]
            cs.append((f - t0, Ei))
        for e in mine:
            if 0 <= jj[e] - t0 < P:
                cs.append((int(jj[e]) - t0, edges[e]["Ej"]))
        out.append(cs)
    return out


def ba(poses, disps, intr, disps_sens, targets, weights, eta, ii, jj, t0, t1, iterations, lm, ep,
       motion_only=False, depth_only=False, dtype=np.float64, quirk=True):
    """Steps 1 to 8.  Returns a dict: poses, disps (updated copies, dtype),
    dx [P, 6], dz [K, HW] (the last iteration's), first = the first
    iteration's dict(H, g, C, w, dx, dz, edges, kx), near, chol_ok."""
    dtype = np.dtype(dtype).type
    poses, disps = np.array(poses, dtype), np.array(disps, dtype)
    sens = np.asarray(disps_sens, dtype)
    ii, jj = [int(i) for i in ii], [int(j) for j in jj]
    N, P = len(ii), t1 - t0
    ht, wd = disps.shape[1:]
    HW = ht * wd
    kx = slots(ii, t0, t1)
    K = len(kx)
    eta = np.asarray(eta, dtype).reshape(K, HW)
    lm, ep = float(np.float32(lm)), float(np.float32(ep))
    near, chol_ok, first = False, True, None
    dx, dz = np.zeros((P, 6), dtype), np.zeros((K, HW), dtype)
    for _ in range(iterations):
        edges = [linearise_edge(poses, disps, intr, targets[e], weights[e], ii[e], jj[e], dtype) for e in range(N)]
        near |= any(ed["near"] for ed in edges)
        # the pose block: rows and columns of fixed poses dropped
        A, a = np.zeros((6 * P, 6 * P)), np.zeros(6 * P)
        for e, ed in enumerate(edges):
            ends = (ii[e] - t0, jj[e] - t0)
            for x, fx_ in enumerate(ends):
                if not 0 <= fx_ < P:
                    continue
                a[6 * fx_:6 * fx_ + 6] += ed["v"][6 * x:6 * x + 6]
                for y, fy_ in enumerate(ends):
                    if 0 <= fy_ < P:
                        A[6 * fx_:6 * fx_ + 6, 6 * fy_:6 * fy_ + 6] += ed["H"][6 * x:6 * x + 6, 6 * y:6 * y + 6]
        H, g = A, a
        C = w = Q = cps = None
        if not motion_only:
            C, w = np.zeros((K, HW), dtype), np.zeros((K, HW), dtype)
            for k, f in enumerate(kx):
                for e in range(N):
                    if ii[e] == f:
                        C[k] += edges[e]["C"]
                        w[k] += edges[e]["bz"]
                m = sens[f].reshape(-1) > 0
                C[k] += np.where(m, dtype(ALPHA), eta[k])
                w[k] -= np.where(m, dtype(ALPHA) * (disps[f].reshape(-1) - sens[f].reshape(-1)), 0).astype(dtype)
            Q = (1 / C).astype(dtype)
            cps = couplings(edges, ii, jj, kx, t0, t1)
            S, s = np.zeros((6 * P, 6 * P)), np.zeros(6 * P)
            for k in range(K):
                qw = Q[k] * w[k]
                for (pa, Ea) in cps[k]:
                    s[6 * pa:6 * pa + 6] += (Ea * qw).sum(1, dtype=np.float64)
                    EaQ = Ea * Q[k]
                    for (pb, Eb) in cps[k]:
                        S[6 * pa:6 * pa + 6, 6 * pb:6 * pb + 6] += (EaQ[:, None, :] * Eb[None, :, :]).sum(
                            2, dtype=np.float64)
            H, g = A - S, a - s
        H = H.copy()
        idx = np.arange(6 * P)
        H[idx, idx] = H[idx, idx] + (ep + lm * H[idx, idx])
        try:
            if not np.isfinite(H).all():
                raise np.linalg.LinAlgError
            Lc = np.linalg.cholesky(H)
            sol = np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        except np.linalg.LinAlgError:
            chol_ok, sol = False, np.zeros(6 * P)
        dx = sol.reshape(P, 6).astype(dtype)    # (float32 mode: rounded once)
        if not motion_only:
            dz = np.zeros((K, HW), dtype)
            for k in range(K):
                acc = np.zeros(HW, dtype)
                for (pa, Ea) in cps[k]:
                    if quirk and pa <= 0:
                        continue    # the recorded quirk: pose t0's own step does not enter dz
                    acc += (Ea * dx[pa][:, None]).sum(0)
                dz[k] = Q[k] * (w[k] - acc)
        if first is None:
            first = dict(H=H, g=g, C=C, w=w, dx=dx.copy(), dz=dz.copy(), edges=edges, kx=kx)
        if motion_only or not depth_only:
            for p in range(P):
                poses[t0 + p] = retract(poses[t0 + p], dx[p], dtype)
        if not motion_only:
            for k, f in enumerate(kx):
                disps[f] += dz[k].reshape(ht, wd)
    return dict(poses=poses, disps=disps, dx=dx, dz=dz, first=first, near=near, chol_ok=chol_ok)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def band_edges(n, radius):
    ii, jj = [], []
    for i in range(n):
        for j in range(n):
            if i != j and abs(i - j) <= radius:
                ii.append(i)
                jj.append(j)
    return ii, jj


def make_case(frames, ii, jj, t0, t1, seed=0, sens=False, ht=None, wd=None):
    """A BA problem on frames ``frames`` (indices into make_inputs()) in that
    order, cropped to the top-left ht x wd pixels: dict of float32 arrays
    poses [num, 7], disps, disps_sens [num, ht, wd], intr [4], targets,
    weights [N, 2, ht, wd], eta [K, ht, wd], int64 ii, jj, and t0, t1.

    targets: the reprojection under poses perturbed by a few 1e-3, plus smooth
    noise; weights in (0, 1] with a block of exact zeros; eta about 0.2 U(0,
    1) + 1e-7; ``sens``: disps_sens positive (the disparity off by about 2 %)
    on half the pixels."""
    P0, D0, intr = make_inputs()
    ht, wd = ht or R.HT, wd or R.WD
    rng = np.random.default_rng(seed)
    poses = np.stack([P0[f] for f in frames]).astype(np.float32)
    disps = np.stack([D0[f][:ht, :wd] for f in frames]).astype(np.float32)
    num, N = len(frames), len(ii)
    true = np.stack([retract(poses[f].astype(np.float64), rng.uniform(-4e-3, 4e-3, 6), np.float64)
                     for f in range(num)])
    v, u = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    targets, weights = np.zeros((N, 2, ht, wd)), np.zeros((N, 2, ht, wd))
    for e in range(N):
        proj, _, _ = project(true[ii[e]], true[jj[e]], disps[ii[e]].astype(np.float64), intr, np.float64,
                             stereo=ii[e] == jj[e])
        ph = rng.uniform(0, 6.28, 2)
        noise = 0.05 * np.stack([np.sin(0.31 * u + 0.17 * v + ph[0]), np.cos(0.23 * u - 0.29 * v + ph[1])])
        targets[e] = proj.reshape(2, ht, wd) + noise
        weights[e] = rng.uniform(0.05, 1.0, (2, ht, wd))
        r0, c0 = int(rng.integers(0, ht - 2)), int(rng.integers(0, wd - 3))
        weights[e, :, r0:r0 + 2, c0:c0 + 3] = 0
    K = len(slots(ii, t0, t1))
    eta = 0.2 * rng.uniform(0, 1, (K, ht, wd)) + 1e-7
    disps_sens = np.zeros_like(disps)
    if sens:
        half = (u + v) % 2 == 0
        disps_sens[:, half] = (disps * (1 + 0.02 * rng.standard_normal(disps.shape)))[:, half]
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    return dict(poses=f32(poses), disps=f32(disps), disps_sens=f32(disps_sens), intr=f32(intr), targets=f32(targets),
                weights=f32(weights), eta=f32(eta), ii=np.array(ii, np.int64), jj=np.array(jj, np.int64),
                t0=t0, t1=t1)


FAR = 9  # make_inputs()'s first far frame: every pixel of a near frame falls under the depth cut in it

_E12 = ([1, 2, 3, 4, 1, 2, 3, 4, 2, 3, 4, 1], [0, 1, 2, 3, 2, 3, 4, 0, 0, 1, 2, 3])


@functools.lru_cache(maxsize=None)
def case(name):
    """The named cases of the tests (cached; treat as read-only)."""
    if name == "a":        # 5 frames, 12 edges, t0 = 1; frame 0 is only ever a target
        return make_case(range(5), _E12[0], _E12[1], 1, 5, seed=1)
    if name == "a_sens":
        return make_case(range(5), _E12[0], _E12[1], 1, 5, seed=1, sens=True)
    if name == "b":        # + a stereo edge and an edge into a far frame (all pixels under the cut)
        return make_case([0, 1, 2, 3, 4, FAR], _E12[0] + [2, 3], _E12[1] + [2, 5], 1, 6, seed=2)
    if name == "c":        # sources below t0: frames 0 and 1 are fixed but their disparities move
        ii, jj = band_edges(5, 2)
        return make_case(range(5), ii, jj, 2, 5, seed=3)
    if name == "small":    # 3 frames, 6 x 8: the dense full-system check
        ii, jj = band_edges(3, 2)
        return make_case(range(3), ii, jj, 1, 3, seed=4, ht=6, wd=8)
    if name.startswith("band"):   # P free frames (the near frames, cycled), 6 x 8 pixels, band graph of radius 2
        P = int(name[4:])
        ii, jj = band_edges(P + 1, 2)
        return make_case([f % R.NFRAMES for f in range(P + 1)], ii, jj, 1, P + 1, seed=5, ht=6, wd=8)
    raise KeyError(name)


def run(c, iterations, lm=1e-4, ep=0.1, **kw):
    return ba(c["poses"], c["disps"], c["intr"], c["disps_sens"], c["targets"], c["weights"], c["eta"], c["ii"],
              c["jj"], c["t0"], c["t1"], iterations, lm, ep, **kw)
