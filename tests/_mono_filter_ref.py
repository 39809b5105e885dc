"""The tracker's DINO-consistency filter of the metric depth prior
(``DepthVideo.filter_high_err_mono_depth``) restated from its definition, in
float64 numpy.  Nothing here imports the package under test.

For each reference frame j and each pixel (x, y) of frame j:

1. X0 = ((x - cx) / fx, (y - cy) / fy, 1), D = disps[j, y, x]; the intrinsics
   are the given 1/8-scale values times 8.
2. X1 = R X0 + t D, (R, t) = pose[idx] pose[j]^-1.
3. Z < 0.1 is replaced by 1 (such a point stays a candidate).
4. u = fx X / Z + cx, v = fy Y / Z + cy, d = D / Z.
5. target (round(u), round(v)), half to even; valid inside the image with d > 0.
6. cosine of frame j's DINO feature at (x, y) and frame idx's at the target,
   both maps upsampled bilinearly (align_corners=False), norms max(|.|, 1e-12).
7. matched: cosine > 0.9.
8. per (j, target) the matched candidate with the largest y W + x wins; w = its d.
9. err = |1 / w - 1 / disps[idx, target]| w (zero disparity: inf); accurate += 1
   if err < 0.02 else inaccurate += 1, once per (j, target).

The mask of idx is cleared where accurate <= 1, inaccurate > 0, disps[idx] > 0.

The ambiguity map marks the targets at which a float32 evaluation may
legitimately decide otherwise: every target a candidate could reach under
either rounding when its u or v lies within ``BAND_PX`` of a rounding boundary,
its Z within ``BAND_Z`` of 0.1 (both values of Z are followed) or its cosine
within ``BAND_COS`` of the threshold, and every target whose winner's err lies
within ``BAND_ERR`` of its threshold.  The float32 ulp at coordinate 75 is
8e-6, so 1e-3 px is over a hundred ulps; 384 fp32 terms at 6e-8 each bound
the cosine's error by about 2.3e-5, a quarter of the band.
"""
from __future__ import annotations

import numpy as np

import _lie_ref as lr

MIN_Z = 0.1
DOWN_SCALE = 8
PATCH = 14
BAND_PX = 1e-3
BAND_COS = 1e-4
BAND_Z = 1e-5
BAND_ERR = 1e-4
AMBIGUITY_CAP = 0.05  # of H W


def _axis(out, inn):
    src = np.maximum((inn / out) * (np.arange(out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), inn - 1)
    i1 = np.minimum(i0 + 1, inn - 1)
    return i0, i1, np.clip(src - i0, 0.0, 1.0)


def upsample(feat, H, W):
    """F.interpolate(mode='bilinear', align_corners=False) of a [hd, wd, C] map to [H, W, C]."""
    feat = np.asarray(feat, np.float64)
    y0, y1, ly = _axis(H, feat.shape[0])
    x0, x1, lx = _axis(W, feat.shape[1])
    ly, lx = ly[:, None, None], lx[None, :, None]
    top = feat[y0][:, x0] * (1 - lx) + feat[y0][:, x1] * lx
    bot = feat[y1][:, x0] * (1 - lx) + feat[y1][:, x1] * lx
    return top * (1 - ly) + bot * ly


def _normalize(f):
    return f / np.maximum(np.sqrt((f * f).sum(-1, keepdims=True)), 1e-12)


def _project(R3, t, X0, D, fx, fy, cx, cy, z_override=None):
    X1 = R3 + t * D[..., None]
    Zraw = X1[..., 2]
    low = Zraw < MIN_Z if z_override is None else z_override
    Z = np.where(low, 1.0, Zraw)
    with np.errstate(all="ignore"):
        u = fx * (X1[..., 0] / Z) + cx
        v = fy * (X1[..., 1] / Z) + cy
        d = D / Z
    return u, v, d, Zraw, low


def _inside(tu, tv, d, H, W):
    with np.errstate(invalid="ignore"):
        return (tu >= 0) & (tu < W) & (tv >= 0) & (tv < H) & (d > 0)


def filter_mono_depth(poses, disps, mask, intrinsics, dino, idx, jj, sim_thresh=0.9, err_thresh=0.02):
    """-> dict(mask [H, W] bool: the new row idx; accurate, inaccurate [H, W]
    int32; ambiguous [H, W] bool; and the generator's statistics: candidates,
    valid, matched, collisions, low_z_valid)."""
    poses, disps = np.asarray(poses, np.float64), np.asarray(disps, np.float64)
    dino = np.asarray(dino, np.float64)
    fx, fy, cx, cy = (float(v) * DOWN_SCALE for v in np.asarray(intrinsics, np.float64).reshape(-1))
    H, W = disps.shape[1:]
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X0 = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1)
    src = (y * W + x).astype(np.int64).reshape(-1)
    fi = _normalize(upsample(dino[idx], H, W))
    Di = disps[idx]
    accurate = np.zeros((H, W), np.int32)
    inaccurate = np.zeros((H, W), np.int32)
    ambiguous = np.zeros((H, W), bool)
    stats = dict(candidates=0, valid=0, matched=0, collisions=0, low_z_valid=0)
    for j in (int(v) for v in np.asarray(jj).reshape(-1)):
        G = lr.mul(poses[idx], lr.inv(poses[j]))
        R3 = lr.rotate(G[3:], X0)
        D = disps[j]
        u, v, d, Zraw, low = _project(R3, G[:3], X0, D, fx, fy, cx, cy)
        tu, tv = np.rint(u), np.rint(v)  # half to even
        valid = _inside(tu, tv, d, H, W)
        tx = np.where(valid, tu, 0).astype(np.int64)
        ty = np.where(valid, tv, 0).astype(np.int64)
        fj = _normalize(upsample(dino[j], H, W))
        cos = (fj * fi[ty, tx]).sum(-1)
        matched = valid & (cos > sim_thresh)
        stats["candidates"] += H * W
        stats["valid"] += int(valid.sum())
        stats["matched"] += int(matched.sum())
        stats["low_z_valid"] += int((valid & low).sum())

        # the winner of each target: the largest source index (ascending order, last write wins)
        m = matched.reshape(-1)
        tgt = (ty * W + tx).reshape(-1)[m]
        win = np.full(H * W, -1, np.int64)
        win[tgt] = src[m]
        hit = win >= 0
        stats["collisions"] += int(m.sum() - hit.sum())
        w = d.reshape(-1)[np.where(hit, win, 0)]
        with np.errstate(all="ignore"):
            err = np.abs(1.0 / w - 1.0 / Di.reshape(-1)) * w
        good = hit & (err < err_thresh)
        accurate += good.reshape(H, W)
        inaccurate += (hit & ~good).reshape(H, W)
        ambiguous |= (hit & (np.abs(err - err_thresh) < BAND_ERR)).reshape(H, W)

        # candidates a float32 evaluation may place, or match, otherwise
        near_z = np.abs(Zraw - MIN_Z) < BAND_Z
        with np.errstate(invalid="ignore"):
            near_px = (np.abs(np.abs(u - np.floor(u)) - 0.5) < BAND_PX) | (np.abs(np.abs(v - np.floor(v)) - 0.5) < BAND_PX)
        near_cos = valid & (np.abs(cos - sim_thresh) < BAND_COS)
        amb = near_z | near_px | near_cos
        for flip in (False, True):
            uu, vv, dd, _, _ = _project(R3, G[:3], X0, D, fx, fy, cx, cy, z_override=(low ^ near_z) if flip else low)
            for du in (-BAND_PX, BAND_PX):
                for dv in (-BAND_PX, BAND_PX):
                    au, av = np.rint(uu + du), np.rint(vv + dv)
                    ok = amb & _inside(au, av, dd, H, W)
                    ambiguous[av[ok].astype(np.int64), au[ok].astype(np.int64)] = True
    new_mask = np.asarray(mask[idx], bool).copy()
    new_mask[(accurate <= 1) & (inaccurate > 0) & (Di > 0)] = False
    return dict(mask=new_mask, accurate=accurate, inaccurate=inaccurate, ambiguous=ambiguous, **stats)


def make_case(H, W, C, poses_xi, depth_scale=None, seed=0, rank=6, noise=0.35, plane=(0.02, -0.03, 2.0), ripple=0.01):
    """Inputs of one synthetic case, as float32 arrays: frames looking at the
    plane n . X = const from the poses exp(poses_xi), with a ``ripple`` on the
    depth; DINO maps a smooth rank-``rank`` field of the WORLD point a cell
    sees plus ``noise``.  ``depth_scale``: {frame: [(y0, y1, x0, x1, factor)]}
    rectangles whose depth is scaled (the moving objects)."""
    rng = np.random.default_rng(seed)
    num = len(poses_xi)
    poses = lr.exp(np.asarray(poses_xi, np.float64))
    fx = fy = 0.9 * W
    cx, cy = 0.5 * W - 0.3, 0.5 * H + 0.2
    intr = np.array([fx, fy, cx, cy]) / DOWN_SCALE
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1)
    a, b, c = plane  # the plane z = a x + b y + c in world coordinates
    nrm = np.array([-a, -b, 1.0])
    hd, wd = H // PATCH, W // PATCH
    depth = np.zeros((num, H, W))
    world = np.zeros((num, H, W, 3))
    for k in range(num):
        c2w = lr.inv(poses[k])
        dirs = lr.rotate(c2w[3:], rays)
        org = c2w[:3]
        s = (c - nrm @ org) / (dirs @ nrm)
        depth[k] = s * (1 + ripple * np.sin(0.9 * x + 0.7 * k) * np.cos(0.8 * y - 0.4 * k))
        world[k] = org + dirs * s[..., None]
    for k, rects in (depth_scale or {}).items():
        for (y0, y1, x0, x1, f) in rects:
            depth[k, y0:y1, x0:x1] *= f
    # the features of a cell: a smooth field of the world point at the cell's centre pixel
    proj = rng.standard_normal((rank, C))
    freq = rng.standard_normal((rank, 3)) * 1.2
    phase = rng.uniform(0, 2 * np.pi, rank)
    dino = np.zeros((num, hd, wd, C))
    for k in range(num):
        yc = np.minimum(((np.arange(hd) + 0.5) * H / hd).astype(int), H - 1)
        xc = np.minimum(((np.arange(wd) + 0.5) * W / wd).astype(int), W - 1)
        pw = world[k][yc][:, xc]
        field = np.cos(pw @ freq.T + phase)
        dino[k] = field @ proj + noise * rng.standard_normal((hd, wd, C))
    f32 = lambda v: np.ascontiguousarray(v, np.float32)  # noqa: E731
    return dict(poses=f32(poses), disps=f32(1.0 / depth), intrinsics=f32(intr), dino=f32(dino))
