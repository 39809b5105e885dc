"""SE3 and the tracker's reprojection restated from their definitions, in numpy.

Every function computes in the dtype of its inputs: float64 arrays give the
oracle the tests compare against, float32 arrays the "same formulas in fp32"
evaluation the GPU tolerances are derived from (tests/test_gpu_lie.py,
tests/test_gpu_reproject.py).  Nothing here imports the package under test.

Conventions: a group element is [..., 7] = (tx, ty, tz, qx, qy, qz, qw), a
tangent vector [..., 6] = (tau, phi), translation part first; the rotation of q
= (u, w) is v -> v + w s + u x s with s = 2 u x v (the quaternion sandwich,
never renormalised); Adj = [[R, [t]x R], [0, R]].

``lietorch_standin()`` wraps these functions as a module with lietorch's
surface over torch CPU tensors, for tests/golden/make_reproject_fixtures.py.
"""
from __future__ import annotations

import types

import numpy as np

SERIES_THETA = 0.25   # a, c, d by series below this angle (next term < 1e-12)
LOG_SMALL = 1e-4      # atan2(n, w) / n by series below this |qv|
MIN_DEPTH = 0.2       # projective_ops.MIN_DEPTH
STEREO = (-0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def _f(x):
    x = np.asarray(x)
    return x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def rotate(q, v):
    """R(q) v for q [..., 4] = (x, y, z, w)"""
    u, w = q[..., :3], q[..., 3:4]
    s = 2 * cross(u, v)
    return v + (w * s + cross(u, s))


def _horner(x, coef):
    r = np.full_like(x, coef[-1])
    for c in coef[-2::-1]:
        r = c + x * r
    return r


def exp(xi):
    xi = _f(xi)
    tau, phi = xi[..., :3], xi[..., 3:]
    th2 = (phi * phi).sum(-1, keepdims=True)
    th = np.sqrt(th2)
    small = th < SERIES_THETA
    ths = np.where(small, 1, th)  # (keeps the unused branch finite)
    a = np.where(small, _horner(th2, [0.5, -1 / 48, 1 / 3840, -1 / 645120]), np.sin(th.dtype.type(0.5) * ths) / ths)
    c = np.where(small, _horner(th2, [1 / 6, -1 / 120, 1 / 5040, -1 / 362880]),
                 (ths - np.sin(ths)) / (ths * ths * ths))
    b = 2 * a * a
    w1 = cross(phi, tau)
    w2 = cross(phi, w1)
    t = tau + (b * w1 + c * w2)
    q = np.concatenate([a * phi, np.cos(th.dtype.type(0.5) * th)], axis=-1)
    return np.concatenate([t, q], axis=-1).astype(xi.dtype)


def log(X):
    X = _f(X)
    t, q = X[..., :3], X[..., 3:]
    q = np.where(q[..., 3:4] < 0, -q, q)
    u, w = q[..., :3], q[..., 3:4]
    n2 = (u * u).sum(-1, keepdims=True)
    n = np.sqrt(n2)
    small = n < LOG_SMALL
    ns = np.where(small, 1, n)
    s = np.where(small, (2 / w) * (1 - n2 / (w * w) / 3), 2 * np.arctan2(ns, w) / ns)
    phi = s * u
    th = s * n
    th2 = th * th
    smallt = th < SERIES_THETA
    th2s = np.where(smallt, 1, th2)
    d = np.where(smallt, _horner(th2, [1 / 12, 1 / 720, 1 / 30240, 1 / 1209600]),
                 (1 - th.dtype.type(0.5) * th * w / ns) / th2s)
    w1 = cross(phi, t)
    w2 = cross(phi, w1)
    tau = t + (d * w2 - th.dtype.type(0.5) * w1)
    return np.concatenate([tau, phi], axis=-1).astype(X.dtype)


def _conj(q):
    return np.concatenate([-q[..., :3], q[..., 3:]], axis=-1)


def inv(X):
    X = _f(X)
    qc = _conj(X[..., 3:])
    return np.concatenate([-rotate(qc, X[..., :3]), qc], axis=-1)


def mul(A, B):
    A, B = np.broadcast_arrays(_f(A), _f(B))
    av, aw, bv, bw = A[..., 3:6], A[..., 6:7], B[..., 3:6], B[..., 6:7]
    qw = aw * bw - (av * bv).sum(-1, keepdims=True)
    qv = aw * bv + bw * av + cross(av, bv)
    t = A[..., :3] + rotate(A[..., 3:], B[..., :3])
    return np.concatenate([t, qv, qw], axis=-1)


def act(X, p):
    """p [..., 3]: R p + t; p [..., 4] = (x, y, z, w): (R xyz + w t, w)"""
    X, p = _f(X), _f(p)
    bs = np.broadcast_shapes(X.shape[:-1], p.shape[:-1])
    X = np.broadcast_to(X, bs + (7,))
    p = np.broadcast_to(p, bs + (p.shape[-1],))
    r = rotate(X[..., 3:], p[..., :3])
    if p.shape[-1] == 3:
        return r + X[..., :3]
    return np.concatenate([r + p[..., 3:4] * X[..., :3], p[..., 3:4]], axis=-1)


def rotation_matrix(q):
    x, y, z, w = (q[..., k] for k in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def matrix(X):
    X = _f(X)
    M = np.zeros(X.shape[:-1] + (4, 4), X.dtype)
    M[..., :3, :3] = rotation_matrix(X[..., 3:])
    M[..., :3, 3] = X[..., :3]
    M[..., 3, 3] = 1
    return M


def _pair(X, a):
    X, a = _f(X), _f(a)
    bs = np.broadcast_shapes(X.shape[:-1], a.shape[:-1])
    return np.broadcast_to(X, bs + (7,)), np.broadcast_to(a, bs + (6,))


def adj(X, a):
    X, a = _pair(X, a)
    rt, rp = rotate(X[..., 3:], a[..., :3]), rotate(X[..., 3:], a[..., 3:])
    return np.concatenate([rt + cross(X[..., :3], rp), rp], axis=-1)


def adjT(X, a):
    X, a = _pair(X, a)
    qc = _conj(X[..., 3:])
    tau = a[..., :3]
    return np.concatenate([rotate(qc, tau), rotate(qc, a[..., 3:] - cross(X[..., :3], tau))], axis=-1)


def retr(X, a):
    return mul(exp(_f(a)), X)


def identity(*batch, dtype=np.float64):
    return np.broadcast_to(np.array([0, 0, 0, 0, 0, 0, 1], dtype), tuple(batch) + (7,)).copy()


# ---------------------------------------------------------------------------
# the reprojection (projective_ops.projective_transform), stated per pixel
# ---------------------------------------------------------------------------
def make_reproject_inputs():
    """6 frames of 30 x 41 pixels, per-frame intrinsics, all 36 ordered pairs
    (ii == jj included); float64 arrays (the tests round them to float32 once
    and feed the same values to the oracle and the GPU)."""
    num, ht, wd = 6, 30, 41
    k = np.arange(num, dtype=np.float64)
    intrinsics = np.array([36.0, 35.0, 19.3, 15.1])[None] * (1 + 0.01 * k)[:, None]
    t = np.stack([0.05 * k, -0.03 * k, 0.15 * k], axis=-1)
    xi = np.concatenate([np.zeros((num, 3)), np.array([0.02, -0.03, 0.05])[None] * k[:, None]], axis=-1)
    poses = np.concatenate([t, exp(xi)[:, 3:]], axis=-1)
    y, x = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    depth = 0.12 + 1.9 * (0.5 + 0.5 * np.sin(0.37 * x[None] + 0.9 * k[:, None, None]) * np.cos(0.23 * y[None]))
    ii, jj = np.meshgrid(np.arange(num), np.arange(num), indexing="ij")
    return dict(poses=poses, disps=1.0 / depth, intrinsics=intrinsics, ii=ii.reshape(-1).astype(np.int64),
                jj=jj.reshape(-1).astype(np.int64))


def relative_transform(poses, ii, jj):
    """G_ij = G_j G_i^-1, the fixed stereo transform where ii == jj"""
    poses = _f(poses)
    G = mul(poses[jj], inv(poses[ii]))
    G[ii == jj] = np.array(STEREO, poses.dtype)
    return G


def reproject(poses, disps, intrinsics, ii, jj, jacobian=False, return_depth=False):
    """dict of coords [E, ht, wd, 2 | 3], valid [E, ht, wd, 1], Z1 [E, ht, wd]
    and, with ``jacobian``, Ji, Jj [E, ht, wd, 2, 6] and Jz [E, ht, wd, 2, 1];
    every output ``name`` comes with ``name + "_mag"``: the same expression on
    the absolute values of its terms (what rounding errors are relative to).
    The transform is applied as a rotation matrix and a translation."""
    poses, disps, intrinsics = _f(poses), _f(disps), _f(intrinsics)
    dt = poses.dtype
    if intrinsics.ndim == 1:
        intrinsics = np.broadcast_to(intrinsics, (poses.shape[0], 4))
    E, (ht, wd) = len(ii), disps.shape[1:]
    G = relative_transform(poses, ii, jj)
    R = rotation_matrix(G[:, 3:])[:, None, None]  # [E, 1, 1, 3, 3]
    t = G[:, None, None, :3]                      # [E, 1, 1, 3]
    Ki, Kj = intrinsics[ii][:, None, None], intrinsics[jj][:, None, None]
    y, x = np.meshgrid(np.arange(ht).astype(dt), np.arange(wd).astype(dt), indexing="ij")
    d = disps[ii]
    X0 = (x[None] - Ki[..., 2]) / Ki[..., 0]
    Y0 = (y[None] - Ki[..., 3]) / Ki[..., 1]
    one = np.ones_like(d)

    def apply(M, tt, a, b, dd):
        return [(M[..., r, 0] * a + M[..., r, 1] * b + M[..., r, 2]) + dd * tt[..., r] for r in range(3)]

    X, Y, Z = apply(R, t, X0, Y0, d)
    mX, mY, mZ = apply(np.abs(R), np.abs(t), np.abs(X0), np.abs(Y0), np.abs(d))
    fx, fy, cx, cy = (Kj[..., c] for c in range(4))
    Zp = np.where(Z < dt.type(0.5 * MIN_DEPTH), one, Z)
    dz = 1 / Zp
    adz = np.abs(dz)
    cs = [fx * (X * dz) + cx, fy * (Y * dz) + cy]
    cm = [fx * (mX * adz) + np.abs(cx), fy * (mY * adz) + np.abs(cy)]
    if return_depth:
        cs.append(d * dz)
        cm.append(np.abs(d) * adz)
    out = dict(coords=np.stack(cs, -1), coords_mag=np.stack(cm, -1),
               valid=((Z > dt.type(MIN_DEPTH)) & (one > dt.type(MIN_DEPTH))).astype(dt)[..., None],
               Z1=Z, Z1_mag=mZ)
    if jacobian:
        def rows(X, Y, Z, d, dz, absval):
            # Jp = [[p00, 0, p02, 0], [0, p11, p12, 0]] times Ja = [d I, -[X1]x; 0]
            o = np.zeros_like(d)
            p00, p11 = fx * dz, fy * dz
            if absval:
                p02, p12 = fx * X * dz * dz, fy * Y * dz * dz
                r0 = [p00 * d, o, p02 * d, p02 * Y, p00 * Z + p02 * X, p00 * Y]
                r1 = [o, p11 * d, p12 * d, p12 * Y + p11 * Z, p12 * X, p11 * X]
            else:
                p02, p12 = -fx * X * dz * dz, -fy * Y * dz * dz
                r0 = [p00 * d, o, p02 * d, p02 * Y, p00 * Z - p02 * X, -p00 * Y]
                r1 = [o, p11 * d, p12 * d, p12 * Y - p11 * Z, -p12 * X, p11 * X]
            return p00, p02, p11, p12, np.stack([np.stack(r0, -1), np.stack(r1, -1)], -2)

        p00, p02, p11, p12, Jj = rows(X, Y, Z, d, dz, False)
        q00, q02, q11, q12, Jj_mag = rows(mX, mY, mZ, np.abs(d), adz, True)
        tx, ty, tz = (t[..., r] for r in range(3))
        out["Jz"] = np.stack([p00 * tx + p02 * tz, p11 * ty + p12 * tz], -1)[..., None]
        out["Jz_mag"] = np.stack([q00 * np.abs(tx) + q02 * np.abs(tz), q11 * np.abs(ty) + q12 * np.abs(tz)],
                                 -1)[..., None]

        def adjT_rows(M, tt, J, sgn):
            u, v = J[..., :3], J[..., 3:]
            c = cross(tt[..., None, :], u) if sgn < 0 else _abs_cross(tt[..., None, :], u)
            v = v + sgn * c
            Mt = np.swapaxes(M, -1, -2)[..., None, :, :]  # [E, 1, 1, 1, 3, 3]
            return np.concatenate([(Mt * u[..., None, :]).sum(-1), (Mt * v[..., None, :]).sum(-1)], -1)

        out["Jj"], out["Jj_mag"] = Jj, Jj_mag
        out["Ji"] = -adjT_rows(R, t, Jj, -1)
        out["Ji_mag"] = adjT_rows(np.abs(R), np.abs(t), Jj_mag, 1)
    return out


def _abs_cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], axis=-1)


def borderline(ref, rel=1e-5):
    """pixels whose depth lies within ``rel`` x magnitude of a branch
    threshold (0.2: valid; 0.1: the depth replaced by 1): fp32 may take the
    other branch there"""
    Z, m = ref["Z1"], ref["Z1_mag"]
    return (np.abs(Z - MIN_DEPTH) <= rel * m) | (np.abs(Z - 0.5 * MIN_DEPTH) <= rel * m)


# ---------------------------------------------------------------------------
# a module with lietorch's surface over torch CPU tensors, computed here
# ---------------------------------------------------------------------------
def lietorch_standin():
    import torch

    def T(a, like):
        return torch.from_numpy(np.ascontiguousarray(a)).to(like.dtype)

    def N(t):
        return t.detach().cpu().double().numpy()

    class SE3:
        manifold_dim, embedded_dim = 6, 7

        def __init__(self, data):
            self.data = data.data if isinstance(data, SE3) else data

        shape = property(lambda self: self.data.shape[:-1])
        device = property(lambda self: self.data.device)
        dtype = property(lambda self: self.data.dtype)

        def __getitem__(self, index):
            if isinstance(index, tuple) and any(i is Ellipsis for i in index):
                index = index + (slice(None),)
            return SE3(self.data[index])

        def inv(self):
            return SE3(T(inv(N(self.data)), self.data))

        def log(self):
            return T(log(N(self.data)), self.data)

        @classmethod
        def exp(cls, x):
            return cls(T(exp(N(x)), x))

        def matrix(self):
            return T(matrix(N(self.data)), self.data)

        def adjT(self, a):
            return T(adjT(N(self.data), N(a)), a)

        def adj(self, a):
            return T(adj(N(self.data), N(a)), a)

        def retr(self, a):
            return SE3(T(retr(N(self.data), N(a)), self.data))

        def __mul__(self, other):
            if isinstance(other, SE3):
                return SE3(T(mul(N(self.data), N(other.data)), self.data))
            return T(act(N(self.data), N(other)), other)

    class Sim3:
        def __init__(self, *a, **k):
            raise NotImplementedError("Sim3")

    m = types.ModuleType("lietorch")
    m.SE3, m.Sim3 = SE3, Sim3
    return m
