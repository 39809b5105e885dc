#!/usr/bin/env python
"""droid_backends on the MI355X path (csrc/droid.hip) against a torch
composition of the same operation on the same GPU.

Device time per call (HIP events, median of repeats after warm-up):

* frame_distance   all 200 x 200 pairs of 200 keyframes at 48 x 64, one-way
                   and fused bidirectional; torch: batched tensor ops over
                   chunks of pairs
* depth_filter     50 frames at 384 x 512; torch: batched tensor ops, one
                   neighbour offset at a time
* corr_index       forward and backward on an fp16 volume [100, 48, 64, 48,
                   64], r = 3; torch: F.grid_sample (zero padding,
                   align_corners=True) on the planes and its autograd backward

Prints one JSON object; ``--out FILE`` also writes it there.  ``--small``
shrinks every problem (a quick check of the tool itself).
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "wildgs-slam-blackwell_amd", "python"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MIN_DEPTH = 0.25


def timed(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def make_frames(num, ht, wd, dev, seed=0):
    """A camera sweeping past a smooth surface: small steps, so neighbouring
    frames see consistent depths."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(num, dtype=torch.float32)
    a = 0.004 * i
    poses = torch.stack([-0.02 * i, 0.01 * torch.cos(i), 0.005 * i, torch.zeros(num), torch.sin(a / 2),
                         torch.zeros(num), torch.cos(a / 2)], 1)
    v, u = torch.meshgrid(torch.arange(ht, dtype=torch.float32), torch.arange(wd, dtype=torch.float32),
                          indexing="ij")
    z = 2 + 0.3 * torch.sin(7 * u / wd + 0.05 * i[:, None, None]) + 0.2 * torch.cos(5 * v / ht)
    disps = (1 / z) * (1 + 0.004 * torch.randn(num, ht, wd, generator=g))
    intr = torch.tensor([0.9 * wd, 0.9 * wd, 0.5 * wd, 0.5 * ht])
    return poses.to(dev).contiguous(), disps.to(dev).contiguous(), intr.to(dev)


# ---- torch compositions -------------------------------------------------------
def quat_rotate(q, X):
    u, w = q[..., None, :3], q[..., None, 3:]
    s = 2 * torch.cross(u.expand_as(X), X, dim=-1)
    return X + w * s + torch.cross(u.expand_as(s), s, dim=-1)


def relative(poses, ii, jj):
    qi, qj, ti, tj = poses[ii, 3:], poses[jj, 3:], poses[ii, :3], poses[jj, :3]
    ax, ay, az, aw = qj.unbind(-1)
    bx, by, bz, bw = (-qi[:, 0], -qi[:, 1], -qi[:, 2], qi[:, 3])
    q = torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)
    return q, tj - quat_rotate(q, ti[:, None, :])[:, 0]


def rays(ht, wd, intr, dev):
    v, u = torch.meshgrid(torch.arange(ht, dtype=torch.float32, device=dev),
                          torch.arange(wd, dtype=torch.float32, device=dev), indexing="ij")
    X = torch.stack([(u - intr[2]) / intr[0], (v - intr[3]) / intr[1], torch.ones_like(u)], -1)
    return X.reshape(-1, 3), u.reshape(-1), v.reshape(-1)


def torch_frame_distance(poses, disps, intr, ii, jj, beta, chunk=4096):
    ht, wd = disps.shape[1:]
    X, u, v = rays(ht, wd, intr, disps.device)
    out = []
    for s in range(0, ii.numel(), chunk):
        i, j = ii[s:s + chunk], jj[s:s + chunk]
        q, t = relative(poses, i, j)
        d = disps[i].reshape(i.numel(), -1, 1)
        accum = valid = 0
        for Y, wgt in ((quat_rotate(q, X[None].expand(i.numel(), -1, -1)) + d * t[:, None], beta),
                       (X[None] + d * t[:, None], 1 - beta)):
            du = intr[0] * Y[..., 0] / Y[..., 2] + intr[2] - u
            dv = intr[1] * Y[..., 1] / Y[..., 2] + intr[3] - v
            ok = Y[..., 2] > MIN_DEPTH
            accum = accum + wgt * torch.where(ok, torch.sqrt(du * du + dv * dv), 0.0).sum(1)
            valid = valid + wgt * ok.sum(1)
        out.append(torch.where(valid / (ht * wd + 1e-8) < 0.75, 1000.0, accum / valid))
    return torch.cat(out)


def torch_depth_filter(poses, disps, intr, inds, thresh):
    num, ht, wd = disps.shape
    X, _, _ = rays(ht, wd, intr, disps.device)
    count = torch.zeros(inds.numel(), ht * wd, device=disps.device)
    d = disps[inds].reshape(inds.numel(), -1, 1)
    flat = disps.reshape(num, -1)
    for neigh in range(6):
        jx = inds - neigh - 1 if neigh < 3 else inds + neigh
        ok = (jx >= 0) & (jx < num)
        jc = jx.clamp(0, num - 1)
        q, t = relative(poses, inds, jc)
        Y = quat_rotate(q, X[None].expand(inds.numel(), -1, -1)) + d * t[:, None]
        uj = intr[0] * Y[..., 0] / Y[..., 2] + intr[2]
        vj = intr[1] * Y[..., 1] / Y[..., 2] + intr[3]
        zj = 1.0 / (d[..., 0] / Y[..., 2])
        u0, v0 = torch.floor(uj), torch.floor(vj)
        inside = (u0 >= 0) & (u0 < wd - 1) & (v0 >= 0) & (v0 < ht - 1) & ok[:, None]
        base = v0.clamp(0, ht - 2).long() * wd + u0.clamp(0, wd - 2).long()
        hit = torch.zeros_like(inside)
        for off in (0, 1, wd, wd + 1):
            hit |= (zj - 1.0 / torch.gather(flat[jc], 1, base + off)).abs() < thresh[:, None]
        count += inside & hit
    return count.reshape(inds.numel(), ht, wd)


def torch_lookup(volume, coords, r):
    n, h1, w1, h2, w2 = volume.shape
    rd = 2 * r + 1
    off = torch.arange(-r, r + 1, dtype=torch.float32, device=volume.device)
    delta = torch.stack(torch.meshgrid(off, off, indexing="ij"), -1).reshape(1, rd, rd, 2)
    g = coords.permute(0, 2, 3, 1).reshape(n * h1 * w1, 1, 1, 2) + delta
    g = torch.stack([2 * g[..., 0] / (w2 - 1) - 1, 2 * g[..., 1] / (h2 - 1) - 1], -1).to(volume.dtype)
    out = F.grid_sample(volume.reshape(n * h1 * w1, 1, h2, w2), g, mode="bilinear", padding_mode="zeros",
                        align_corners=True)
    return out.reshape(n, h1, w1, rd, rd).permute(0, 3, 4, 1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import droid_backends
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}

    def row(name, ours, theirs, **extra):
        res[name] = dict(hip_ms=ours, torch_ms=theirs, torch_over_hip=theirs / ours, **extra)

    # frame_distance
    nkf = 24 if args.small else 200
    poses, disps, intr = make_frames(nkf, 48, 64, dev)
    ii, jj = (a.reshape(-1).contiguous() for a in torch.meshgrid(torch.arange(nkf, device=dev),
                                                                  torch.arange(nkf, device=dev), indexing="ij"))
    ours = droid_backends.frame_distance(poses, disps, intr, ii, jj, 0.3)
    theirs = torch_frame_distance(poses, disps, intr, ii, jj, 0.3)
    agree = float(((ours - theirs).abs() <= 1e-3 * theirs.abs() + 1e-4).float().mean())
    t_one = timed(lambda: droid_backends.frame_distance(poses, disps, intr, ii, jj, 0.3))
    t_two = timed(lambda: (droid_backends.frame_distance(poses, disps, intr, ii, jj, 0.3),
                           droid_backends.frame_distance(poses, disps, intr, jj, ii, 0.3)))
    t_fused = timed(lambda: droid_backends.frame_distance(poses, disps, intr, ii, jj, 0.3, bidirectional=True))
    t_torch = timed(lambda: torch_frame_distance(poses, disps, intr, ii, jj, 0.3), reps=5, warm=1)
    row("frame_distance", t_one, t_torch, pairs=ii.numel(), frame="48x64", agree=agree)
    row("frame_distance_bidirectional", t_fused, 2 * t_torch, two_launches_ms=t_two)

    # depth_filter
    nf, ht, wd = (8, 96, 128) if args.small else (50, 384, 512)
    poses, disps, intr = make_frames(nf, ht, wd, dev, seed=1)
    inds = torch.arange(nf, device=dev)
    th = (0.01 * (1 / disps).mean(dim=[1, 2])).contiguous()
    ours = droid_backends.depth_filter(poses, disps, intr, inds, th)
    theirs = torch_depth_filter(poses, disps, intr, inds, th)
    agree = float((ours == theirs).float().mean())
    row("depth_filter", timed(lambda: droid_backends.depth_filter(poses, disps, intr, inds, th)),
        timed(lambda: torch_depth_filter(poses, disps, intr, inds, th), reps=5, warm=1),
        frames=nf, frame=f"{ht}x{wd}", agree=agree, mean_count=float(ours.mean()))

    # corr_index
    n, r = (4 if args.small else 100), 3
    g = torch.Generator(device=dev).manual_seed(2)
    volume = torch.randn(n, 48, 64, 48, 64, device=dev, dtype=torch.float16, generator=g)
    v, u = torch.meshgrid(torch.arange(48, dtype=torch.float32, device=dev),
                          torch.arange(64, dtype=torch.float32, device=dev), indexing="ij")
    # the pixel's own position plus a flow of a few pixels (some leave the plane)
    coords = torch.stack([u, v])[None] + 4 * torch.randn(n, 2, 48, 64, device=dev, generator=g)
    coords = coords.contiguous()
    ours = droid_backends.corr_index_forward(volume, coords, r)[0]
    # (agreement against an fp32 grid_sample of two volumes: in fp16 torch also
    # rounds the sampling grid itself)
    theirs = torch_lookup(volume[:2].float(), coords[:2], r)
    agree = float(((ours[:2].float() - theirs).abs() <= 2e-3 * theirs.abs() + 1e-3).float().mean())
    grad = torch.randn_like(ours)
    row("corr_index_forward", timed(lambda: droid_backends.corr_index_forward(volume, coords, r)),
        timed(lambda: torch_lookup(volume, coords, r)), volume=list(volume.shape), dtype="float16", radius=r,
        agree=agree)
    vol_g = volume.clone().requires_grad_(True)

    def torch_bwd():
        out = torch_lookup(vol_g, coords, r)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g_, = torch.autograd.grad(out, vol_g, grad)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), g_

    ts = sorted(torch_bwd()[0] for _ in range(5))
    g_ours = droid_backends.corr_index_backward(volume, coords, grad, r)[0]
    v32 = volume[:2].float().requires_grad_(True)
    g_theirs, = torch.autograd.grad(torch_lookup(v32, coords[:2], r), v32, grad[:2].float())
    agree = float(((g_ours[:2].float() - g_theirs).abs() <= 2e-3 * g_theirs.abs() + 1e-3).float().mean())
    del g_theirs, v32
    row("corr_index_backward", timed(lambda: droid_backends.corr_index_backward(volume, coords, grad, r)),
        ts[len(ts) // 2], agree=agree, note="torch: the autograd backward of grid_sample alone, forward excluded")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
