#!/usr/bin/env python
"""wgsr.frontend.filter_mono_depth (csrc/droid_mono_filter.hip: four launches,
no full-resolution feature map) against the same steps written eagerly in torch
(the pattern of DepthVideo.filter_high_err_mono_depth: each frame's DINO map
upsampled to full resolution, gathered by boolean masks, scattered with
``index_put``), on the same GPU and build.

One call at the tracker's shape: 384 x 512 pixels, 6 reference frames, C = 384
(27 x 36 cells), the DINO maps on the device for both forms (the eager form is
spared the reference's host-to-device copy of the upsampled maps).

* ``call_ms``  device time per call as the caller sees it: HIP events around a
               batch of back-to-back calls (after warm-up), the median over
               repeats, fused and eager batches alternating.
* ``agree``    the share of pixels at which the two masks / count maps are
               equal.  Not 1: the eager form's ``index_put`` with duplicate
               indices picks an arbitrary winner, and its cosines are summed in
               another order.
* ``unique_bytes`` what the fused call has to move: the winner words (written,
               hit by the atomics, read), the Gram matrices (written once, read
               from cache), 13 cell maps, 7 disparity maps, the mask row.

Prints one JSON object; ``--out FILE`` also writes it there.  ``--small``
shrinks the problem (a quick check of the tool itself).
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "wildgs-slam-blackwell_amd", "python"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy
MIN_Z = 0.1


def eager(poses, disps, mask, intrinsics, dino, idx, jj, sim_thresh=0.9, err_thresh=0.02):
    """the filter's steps, one torch expression each; -> (accurate, inaccurate)"""
    from lietorch import SE3
    H, W = disps.shape[1:]
    dev = poses.device
    E = jj.numel()
    fx, fy, cx, cy = (intrinsics * 8).unbind(-1)
    G = SE3(poses[None])
    ii = torch.full((E,), idx, dtype=torch.int64, device=dev)
    Gji = G[:, ii] * G[:, jj].inv()
    y, x = torch.meshgrid(torch.arange(H, device=dev).float(), torch.arange(W, device=dev).float(), indexing="ij")
    D = disps[jj][None]
    one = torch.ones_like(D)
    X0 = torch.stack([((x - cx) / fx).expand_as(D), ((y - cy) / fy).expand_as(D), one, D], dim=-1)
    X, Y, Z, Dd = (Gji[:, :, None, None] * X0).unbind(-1)
    iz = 1.0 / torch.where(Z < MIN_Z, one, Z)
    x1 = torch.stack([fx * (X * iz) + cx, fy * (Y * iz) + cy, Dd * iz], dim=-1)
    r = torch.round(x1[..., :2]).long()
    valid = (r[..., 1] >= 0) & (r[..., 1] < H) & (r[..., 0] >= 0) & (r[..., 0] < W) & (x1[..., 2] > 0)
    Di = disps[idx]
    accurate, inaccurate = torch.zeros_like(Di), torch.zeros_like(Di)
    i_dino = F.interpolate(dino[idx].permute(2, 0, 1).unsqueeze(0), (H, W), mode="bilinear").squeeze(0)
    for k in range(E):
        j_dino = F.interpolate(dino[jj[k]].permute(2, 0, 1).unsqueeze(0), (H, W), mode="bilinear").squeeze(0)
        vm = valid[0, k]
        vx, vy = r[0, k, ..., 0][vm], r[0, k, ..., 1][vm]
        sim = F.normalize(j_dino[:, vm], p=2, dim=0).mul(F.normalize(i_dino[:, vy, vx], p=2, dim=0)).sum(dim=0)
        mm = sim > sim_thresh
        proj = torch.zeros_like(Di)
        mx, my = vx[mm], vy[mm]
        proj[my, mx] = x1[0, k][vm][mm][..., 2]
        err = torch.abs(1 / proj[my, mx] - 1 / Di[my, mx]) * proj[my, mx]
        ok = err < err_thresh
        accurate[my[ok], mx[ok]] += 1
        inaccurate[my[~ok], mx[~ok]] += 1
    mask[idx][(accurate <= 1) & (inaccurate > 0) & (Di > 0)] = False
    return accurate.int(), inaccurate.int()


def make_inputs(frames, H, W, C, dev, seed=3):
    from lietorch import SE3
    g = torch.Generator(device=dev).manual_seed(seed)
    hd, wd = H // 14, W // 14
    xi = 0.03 * torch.randn(frames, 6, device=dev, generator=g)
    xi[0] = 0
    with torch.no_grad():
        poses = SE3.exp(xi).data.contiguous()
    y, x = torch.meshgrid(torch.arange(H, device=dev).float(), torch.arange(W, device=dev).float(), indexing="ij")
    k = torch.arange(frames, device=dev).float()[:, None, None]
    depth = 2.0 + 0.3 * torch.sin(0.02 * x + 0.3 * k) * torch.cos(0.03 * y) + 0.1 * k
    depth[1, H // 4:H // 2, W // 4:W // 2] *= 0.7   # a moving object
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5], device=dev) / 8
    # a smooth low-rank field over the cells, shared by the frames, plus noise
    cy, cx = torch.meshgrid(torch.arange(hd, device=dev).float(), torch.arange(wd, device=dev).float(), indexing="ij")
    rank = 6
    freq = torch.randn(rank, 2, device=dev, generator=g) * 0.25
    field = torch.cos(cy[..., None] * freq[:, 0] + cx[..., None] * freq[:, 1])
    proj = torch.randn(rank, C, device=dev, generator=g)
    dino = (field @ proj)[None] + 0.55 * torch.randn(frames, hd, wd, C, device=dev, generator=g)
    return poses, (1.0 / depth).contiguous(), intr.contiguous(), dino.contiguous()


def batch_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--eager-calls", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    from wgsr import frontend
    dev = torch.device("cuda:0")
    H, W, C, E = (58, 75, 32, 3) if args.small else (384, 512, 384, 6)
    frames = E + 1
    poses, disps, intr, dino = make_inputs(frames, H, W, C, dev)
    jj = torch.arange(1, frames, device=dev)
    start = torch.ones(frames, H, W, dtype=torch.bool, device=dev)
    m_f, m_e = start.clone(), start.clone()
    with torch.no_grad():
        fused = lambda: frontend.filter_mono_depth(poses, disps, m_f, intr, dino, 0, jj, return_counts=True,  # noqa: E731
                                                   check=False)
        eag = lambda: eager(poses, disps, m_e, intr, dino, 0, jj)  # noqa: E731
        (fa, fi), (ea, ei) = fused(), eag()
        torch.cuda.synchronize()
        agree = dict(mask=float((m_f == m_e).float().mean()), accurate=float((fa == ea).float().mean()),
                     inaccurate=float((fi == ei).float().mean()))
        cleared = dict(fused=int((~m_f[0]).sum()), eager=int((~m_e[0]).sum()))
        for _ in range(2):
            fused()
            eag()
        torch.cuda.synchronize()
        tf, te = [], []
        for _ in range(args.reps):
            tf.append(batch_ms(fused, args.calls))
            te.append(batch_ms(eag, args.eager_calls))
    tf.sort()
    te.sort()
    stat = lambda t: dict(median=t[len(t) // 2], min=t[0], max=t[-1])  # noqa: E731
    n = (H // 14) * (W // 14)
    nbytes = dict(winner_words=E * H * W * 8, gram_matrices=(2 * E + 1) * n * n * 4,
                  cell_maps=(2 * E + 1) * n * C * 4, disparities=(E + 1) * H * W * 4, mask_row=H * W)
    unique = 3 * nbytes["winner_words"] + nbytes["gram_matrices"] + sum(nbytes[k] for k in ("cell_maps", "disparities",
                                                                                              "mask_row"))
    res = {"device": torch.cuda.get_device_name(0),
           "problem": dict(H=H, W=W, C=C, references=E, cells=n, calls_per_batch=args.calls,
                           eager_calls_per_batch=args.eager_calls, repeats=args.reps),
           "fused_call_ms": stat(tf), "eager_call_ms": stat(te), "eager_over_fused": te[len(te) // 2] / tf[len(tf) // 2],
           "agree": agree, "cleared_pixels": cleared, "bytes": nbytes, "unique_bytes": unique,
           "byte_model_floor_ms": 1e3 * unique / HBM_BYTES_PER_S,
           "gram_flop": 2 * (2 * E + 1) * n * n * C}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
