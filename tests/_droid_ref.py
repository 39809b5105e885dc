"""float64 numpy restatement of the ``droid_backends`` ops built in
csrc/droid.hip, and the generator of the inputs their tests share.

The oracle states the ops from their definition: parity
with the reference's CUDA binary is unpinned, as for the rasteriser.

Conventions: poses [num, 7] = (tx, ty, tz, qx, qy, qz, qw), world to camera;
disps [num, ht, wd]; intrinsics (fx, fy, cx, cy); pixel (u = column, v = row)
with disparity d is X = ((u - cx) / fx, (v - cy) / fy, 1, d); i -> j is
q_ij = q_j conj(q_i), t_ij = t_j - R(q_ij) t_i, Y = (R(q_ij) X_xyz + d t_ij, d).
"""
import functools

import numpy as np

MIN_DEPTH = 0.25
HT, WD, NFRAMES = 30, 41, 9
INTRINSICS = (36.0, 35.0, 19.3, 15.1)
FAR_TZ = (-1.9, -1.4, -1.7)
BETA = 0.3
FILTER_THRESH = 0.01
VISIBLE_NUM = 2
# a pixel is borderline when a projection lies this close to an integer, or
# the best depth difference this close to the threshold
BORDER_UV, BORDER_DIFF = 2e-4, 2e-5
BORDER_MIN_DEPTH = 1e-5


# ---------------------------------------------------------------------------
# rigid transforms
# ---------------------------------------------------------------------------
def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def rot_delta(q, X):
    """R(q) X - X for points X [..., 3], as DROID's actSO3 states the
    rotation: s = 2 (u x X), delta = w s + u x s with q = (u, w)."""
    u, w = np.asarray(q[:3], np.float64), q[3]
    s = 2 * np.cross(u, X)
    return w * s + np.cross(u, s)


def rotate(q, X):
    return X + rot_delta(q, X)


def relative(pose_i, pose_j):
    """(q_ij, t_ij) taking frame i's camera coordinates to frame j's."""
    pi, pj = np.asarray(pose_i, np.float64), np.asarray(pose_j, np.float64)
    qi = pi[3:]
    q = quat_mul(pj[3:], np.array([-qi[0], -qi[1], -qi[2], qi[3]]))
    return q, pj[:3] - rotate(q, pi[:3])


def rays(ht, wd, intr):
    fx, fy, cx, cy = intr
    v, u = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    return np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1), u, v


# ---------------------------------------------------------------------------
# the shared inputs
# ---------------------------------------------------------------------------
def _surface(x, y):
    return 2 + 0.3 * np.sin(1.3 * x) + 0.2 * np.cos(1.7 * y)


@functools.lru_cache(maxsize=None)
def make_inputs():
    """poses [12, 7], disps [12, HT, WD] (float32), intrinsics [4]: nine
    frames looking at one smooth surface (a block of each frame scaled to be
    inconsistent with its neighbours, 0.4 % noise), then three far frames
    for frame_distance."""
    intr = np.array(INTRINSICS, np.float64)
    X, _, _ = rays(HT, WD, intr)
    poses = np.zeros((NFRAMES + 3, 7))
    disps = np.zeros((NFRAMES + 3, HT, WD))
    for i in range(NFRAMES):
        a = 0.012 * i
        poses[i] = (-0.05 * i, 0.01 * (-1) ** i, 0.015 * i, 0, np.sin(a / 2), 0, np.cos(a / 2))
        q, t = poses[i, 3:], poses[i, :3]
        q_inv = np.array([-q[0], -q[1], -q[2], q[3]])
        z = np.full((HT, WD), 2.0)
        for _ in range(60):
            Pw = rotate(q_inv, X * z[..., None] - t)  # R^-1 (ray z - t)
            z = z + 0.8 * (_surface(Pw[..., 0], Pw[..., 1]) - Pw[..., 2])
        disps[i] = 1.0 / z
        disps[i, 3 + 2 * i:3 + 2 * i + 7, 5 + 3 * i:5 + 3 * i + 9] *= 1.4
    disps[:NFRAMES] *= 1 + 0.004 * np.random.default_rng(0).standard_normal((NFRAMES, HT, WD))
    for k, tz in enumerate(FAR_TZ):
        poses[NFRAMES + k] = (0, 0, tz, 0, 0, 0, 1)
        disps[NFRAMES + k] = disps[k]
    # the kernels read float32: the oracle works on the same rounded values
    return poses.astype(np.float32), disps.astype(np.float32), intr.astype(np.float32)


def filter_thresh(disps, inds):
    """thresh * mean depth of each frame, float32 like the caller's tensor."""
    d = np.asarray(disps, np.float64)[np.asarray(inds)]
    return (FILTER_THRESH * (1.0 / d).mean(axis=(1, 2))).astype(np.float32)


# ---------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------
def frame_distance(poses, disps, intr, ii, jj, beta):
    """(dist [n], ratio [n], near [n]): ratio = valid / total; near = some
    transformed depth lies within BORDER_MIN_DEPTH of MIN_DEPTH."""
    poses, disps, intr = (np.asarray(a, np.float64) for a in (poses, disps, intr))
    fx, fy = intr[:2]
    ht, wd = disps.shape[1:]
    X, _, _ = rays(ht, wd, intr)
    total = ht * wd
    dist, ratio, near = np.zeros(len(ii)), np.zeros(len(ii)), np.zeros(len(ii), bool)
    for k, (i, j) in enumerate(zip(ii, jj)):
        q, t = relative(poses[i], poses[j])
        d = disps[i]
        accum = valid = 0.0
        # M = Y - X: the flow fx Y0 / Y2 + cx - u is fx (M0 - X0 M2) / Y2 (X2 =
        # 1), stated without the cancellation against u (exactly 0 for i = j)
        for M, wgt in ((rot_delta(q, X) + d[..., None] * t, beta), (d[..., None] * t, 1 - beta)):
            Y2 = 1 + M[..., 2]
            ok = Y2 > MIN_DEPTH
            near[k] |= bool((np.abs(Y2 - MIN_DEPTH) < BORDER_MIN_DEPTH).any())
            with np.errstate(divide="ignore", invalid="ignore"):
                flow = np.hypot(fx * (M[..., 0] - X[..., 0] * M[..., 2]) / Y2,
                                fy * (M[..., 1] - X[..., 1] * M[..., 2]) / Y2)
            accum += wgt * flow[ok].sum()
            valid += wgt * ok.sum()
        ratio[k] = valid / total
        dist[k] = 1000.0 if valid / (total + 1e-8) < 0.75 else accum / valid
    return dist, ratio, near


def depth_filter(poses, disps, intr, inds, thresh):
    """(count [m, ht, wd], borderline [m, ht, wd])."""
    poses, disps, intr = (np.asarray(a, np.float64) for a in (poses, disps, intr))
    thresh = np.asarray(thresh, np.float64)
    fx, fy, cx, cy = intr
    num, ht, wd = disps.shape
    X, _, _ = rays(ht, wd, intr)
    count = np.zeros((len(inds), ht, wd))
    border = np.zeros((len(inds), ht, wd), bool)
    for b, ix in enumerate(inds):
        d = disps[ix]
        for neigh in range(6):
            jx = ix - neigh - 1 if neigh < 3 else ix + neigh
            if jx < 0 or jx >= num:
                continue
            q, t = relative(poses[ix], poses[jx])
            Y = rotate(q, X) + d[..., None] * t
            uj, vj = fx * Y[..., 0] / Y[..., 2] + cx, fy * Y[..., 1] / Y[..., 2] + cy
            zj = 1.0 / (d / Y[..., 2])
            border[b] |= (np.abs(uj - np.round(uj)) < BORDER_UV) | (np.abs(vj - np.round(vj)) < BORDER_UV)
            u0, v0 = np.floor(uj).astype(np.int64), np.floor(vj).astype(np.int64)
            inside = (u0 >= 0) & (u0 < wd - 1) & (v0 >= 0) & (v0 < ht - 1)
            uc, vc = np.clip(u0, 0, wd - 2), np.clip(v0, 0, ht - 2)
            best = np.full((ht, wd), np.inf)
            for dv in (0, 1):
                for du in (0, 1):
                    best = np.minimum(best, np.abs(zj - 1.0 / disps[jx][vc + dv, uc + du]))
            count[b] += inside & (best < thresh[b])
            border[b] |= inside & (np.abs(best - thresh[b]) < BORDER_DIFF)
    return count, border


def iproj(poses, disps, intr):
    poses, disps, intr = (np.asarray(a, np.float64) for a in (poses, disps, intr))
    X, _, _ = rays(disps.shape[1], disps.shape[2], intr)
    out = np.zeros(disps.shape + (3,))
    for f in range(disps.shape[0]):
        d = disps[f][..., None]
        out[f] = (rotate(poses[f, 3:], X) + d * poses[f, :3]) / d
    return out


def valid_depth_mask(disps, inds, count, visible_num=VISIBLE_NUM, exclude=None):
    """(mask [m, ht, wd], median [m]) of update_valid_depth_mask, from a
    count; pixels of ``exclude`` take no part in the median.  The median is
    torch.nanmedian's: the lower of the two middle values."""
    depth = 1.0 / np.asarray(disps, np.float64)[np.asarray(inds)]
    keep = np.asarray(count) >= visible_num
    mask, med = np.zeros(depth.shape, bool), np.full(len(depth), np.nan)
    for b in range(len(depth)):
        sel = keep[b] if exclude is None else keep[b] & ~exclude[b]
        vals = np.sort(depth[b][sel])
        if len(vals):
            med[b] = vals[(len(vals) - 1) // 2]
            mask[b] = keep[b] & (depth[b] < 3 * med[b])
    return mask, med


# ---------------------------------------------------------------------------
# correlation lookup
# ---------------------------------------------------------------------------
def _taps(coords, n, y, x, r):
    """floor and fractional part of the lookup centre of position (n, y, x)."""
    x0, y0 = float(coords[n, 0, y, x]), float(coords[n, 1, y, x])
    fx, fy = np.floor(x0), np.floor(y0)
    return int(fx), int(fy), x0 - fx, y0 - fy


def corr_index_forward(volume, coords, r):
    """corr [n, 2r+1, 2r+1, h1, w1] in float64: the bilinear sample of
    volume[n, y, x] at (x0 + i - r, y0 + j - r), zero outside the plane."""
    volume, coords = np.asarray(volume, np.float64), np.asarray(coords, np.float64)
    N, h1, w1, h2, w2 = volume.shape
    rd = 2 * r + 1
    corr = np.zeros((N, rd, rd, h1, w1))

    def at(plane, yy, xx):
        return plane[yy, xx] if 0 <= yy < h2 and 0 <= xx < w2 else 0.0

    for n in range(N):
        for y in range(h1):
            for x in range(w1):
                fx, fy, dx, dy = _taps(coords, n, y, x, r)
                plane = volume[n, y, x]
                for i in range(rd):
                    for j in range(rd):
                        xx, yy = fx + i - r, fy + j - r
                        corr[n, i, j, y, x] = ((1 - dx) * (1 - dy) * at(plane, yy, xx)
                                               + dx * (1 - dy) * at(plane, yy, xx + 1)
                                               + (1 - dx) * dy * at(plane, yy + 1, xx)
                                               + dx * dy * at(plane, yy + 1, xx + 1))
    return corr


def corr_index_backward(shape, coords, corr_grad, r):
    """(volume_grad, touched): the adjoint of corr_index_forward applied to
    corr_grad, and the elements some tap lands on."""
    coords, corr_grad = np.asarray(coords, np.float64), np.asarray(corr_grad, np.float64)
    N, h1, w1, h2, w2 = shape
    rd = 2 * r + 1
    grad = np.zeros(shape)
    touched = np.zeros(shape, bool)
    for n in range(N):
        for y in range(h1):
            for x in range(w1):
                fx, fy, dx, dy = _taps(coords, n, y, x, r)
                for i in range(rd):
                    for j in range(rd):
                        g = corr_grad[n, i, j, y, x]
                        xx, yy = fx + i - r, fy + j - r
                        for (ty, tx, wgt) in ((yy, xx, (1 - dx) * (1 - dy)), (yy, xx + 1, dx * (1 - dy)),
                                              (yy + 1, xx, (1 - dx) * dy), (yy + 1, xx + 1, dx * dy)):
                            if 0 <= ty < h2 and 0 <= tx < w2:
                                grad[n, y, x, ty, tx] += wgt * g
                                touched[n, y, x, ty, tx] = True
    return grad, touched


def make_lookup_inputs(n=3, h1=5, w1=7, h2=6, w2=9, seed=1):
    """volume [n, h1, w1, h2, w2] (float64, O(1) values) and coords [n, 2, h1,
    w1] (float32) covering interior points, exact integers, every border
    straddled, negative values and centres more than r + 1 (r <= 3) outside
    the plane."""
    rng = np.random.default_rng(seed)
    volume = rng.standard_normal((n, h1, w1, h2, w2))
    cx = rng.uniform(0.5, w2 - 1.5, (n, h1, w1))
    cy = rng.uniform(0.5, h2 - 1.5, (n, h1, w1))
    special = [(2.0, 3.0), (0.0, 0.0), (w2 - 1.0, h2 - 1.0),            # exact integers
               (-0.5, 2.25), (w2 - 0.5, 2.25), (3.25, -0.5), (3.25, h2 - 0.5),  # every border straddled
               (-0.25, -0.75), (w2 - 0.25, h2 - 0.75),                    # corners
               (-2.5, 1.5), (1.5, -3.25), (-1.0, -1.0),                   # negative
               (-5.5, 2.0), (w2 + 4.5, 2.0), (3.0, -6.25), (3.0, h2 + 4.25),  # beyond r + 1: all-zero window
               (-40.0, -40.0), (1000.5, 3.0)]
    flat_x, flat_y = cx.reshape(n, -1), cy.reshape(n, -1)
    for k, (sx, sy) in enumerate(special):
        flat_x[k % n, (k // n) * 3 % (h1 * w1)] = sx
        flat_y[k % n, (k // n) * 3 % (h1 * w1)] = sy
    coords = np.stack([flat_x.reshape(n, h1, w1), flat_y.reshape(n, h1, w1)], 1).astype(np.float32)
    return volume, coords
