#!/usr/bin/env python
"""droid_backends.altcorr_* and wgsr.frontend.AltCorrBlock on the MI355X
(csrc/droid_altcorr.hip) against what they replace, on the same GPU.

Device time per call (HIP events, median of repeats after warm-up) and peak
device memory above the inputs (``torch.cuda.max_memory_allocated``), at 48 x
64 maps, C = 128, r = 3, 96 edges, coordinates = the pixel's own position
plus a flow of about 4 px -- "rough": independent per pixel (4 x a standard
normal, as tools/bench_droid.py draws it; neighbouring windows then overlap
little), and "smooth": a low-frequency field of that amplitude plus 0.25 px of
noise, which is what a reprojection gives:

* forward   the plain fp32 ``altcorr_forward`` against the composition
            "all-pairs ``torch.matmul`` + ``corr_index_forward``", which
            stores the [96, 48, 64, 48, 64] volume the op exists to avoid
* block     ``AltCorrBlock`` on an fp16 feature buffer (four levels, one
            indexed launch each) against the update loop's call pattern built
            on the plain op: per level gather the edges' maps, convert them to
            fp32, scale the coordinates, call, permute, and concatenate
* backward  ``altcorr_backward`` against torch autograd through the
            composition (its backward alone, the forward excluded)

``floors`` are derived from the shapes, not measured: the FMAs the op needs at
the fp32 vector peak, and the unique bytes of maps, coordinates and output at
the measured HBM copy rate.  Prints one JSON object; ``--out FILE`` also writes
it there.  ``--small`` shrinks every problem (a quick check of the tool itself).
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "wildgs-slam-blackwell_amd", "python"))

import torch  # noqa: E402

PEAK_FP32_FLOPS = 157.3e12  # vector fp32, datasheet
HBM_BYTES_PER_S = 6.29e12   # measured float4 copy


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


def peak_bytes(fn):
    """Peak device memory of one call above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def floors(entries, hw, taps, c, levels, in_bytes, out_bytes):
    fma = entries * hw * taps * c * levels
    return dict(fma=fma, fma_floor_ms=2e3 * fma / PEAK_FP32_FLOPS, unique_bytes=in_bytes + out_bytes,
                traffic_floor_ms=1e3 * (in_bytes + out_bytes) / HBM_BYTES_PER_S)


def agree(a, b, rel=1e-4, tol=1e-3):
    return float(((a.float() - b.float()).abs() <= rel * b.float().abs() + tol).float().mean())


class VolumeLookup(torch.autograd.Function):
    """corr_index_forward / corr_index_backward as one differentiable op."""

    @staticmethod
    def forward(ctx, volume, coords, r):
        import droid_backends
        ctx.save_for_backward(volume, coords)
        ctx.r = r
        return droid_backends.corr_index_forward(volume, coords, r)[0]

    @staticmethod
    def backward(ctx, grad):
        import droid_backends
        volume, coords = ctx.saved_tensors
        return droid_backends.corr_index_backward(volume, coords, grad.contiguous(), ctx.r)[0], None, None


def composition(f1, f2, coords, r):
    """[E, (2r+1)^2, H, W] from maps [E, H, W, C] and coords [E, 1, H, W, 2]
    through the stored all-pairs volume."""
    E, H, W, C = f1.shape
    volume = torch.matmul(f1.view(E, H * W, C), f2.view(E, H * W, C).transpose(1, 2)).view(E, H, W, H, W)
    return VolumeLookup.apply(volume, coords[:, 0].permute(0, 3, 1, 2).contiguous(), r).view(E, -1, H, W)


def call_pattern(block, coords, ii, jj):
    """The update loop's per-level pattern on the plain op, for coords [B, E,
    H, W, 2]: gathered fp32 copies of the maps, scaled coordinates, one call
    per level, permute, concatenate."""
    import droid_backends
    B, E, H, W, _ = coords.shape
    parts = []
    for i, level in enumerate(block.pyramid):
        m1 = block.pyramid[0][:, ii].reshape(B * E, H, W, -1).float()
        m2 = level[:, jj].reshape((B * E,) + level.shape[2:]).float()
        scaled = (coords / 2 ** i).reshape(B * E, 1, H, W, 2).contiguous()
        corr, = droid_backends.altcorr_forward(m1, m2, scaled, block.radius)
        parts.append(corr.view(B, E, 1, -1, H, W).permute(0, 1, 3, 4, 5, 2))
    return torch.cat(parts, 2).squeeze(-1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import droid_backends
    from wgsr.frontend import AltCorrBlock
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0)}
    E, H, W, C, r, frames, levels = (6, 16, 24, 128, 3, 5, 4) if args.small else (96, 48, 64, 128, 3, 24, 4)
    rd2, taps = (2 * r + 1) ** 2, (2 * r + 2) ** 2
    g = torch.Generator(device=dev).manual_seed(4)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev),
                          torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
    grid = torch.stack([u, v], -1)[None, None]
    coords = (grid + 4 * torch.randn(E, 1, H, W, 2, device=dev, generator=g)).contiguous()
    phase = 6.28 * torch.rand(E, 1, 1, 1, 2, device=dev, generator=g)
    wave = torch.stack([torch.sin(5 * u / W + 3 * v / H), torch.cos(4 * v / H - 2 * u / W)], -1)[None, None]
    smooth = (grid + 4 * torch.sin(wave + phase) + 0.25 * torch.randn(E, 1, H, W, 2, device=dev, generator=g)).contiguous()
    res["problem"] = dict(edges=E, maps=f"{H}x{W}", channels=C, radius=r, levels=levels, frames=frames)

    # (a) the plain fp32 forward against the stored-volume composition
    f1 = torch.randn(E, H, W, C, device=dev, generator=g)
    f2 = torch.randn(E, H, W, C, device=dev, generator=g)
    ours = droid_backends.altcorr_forward(f1, f2, coords, r)[0]
    theirs = composition(f1, f2, coords, r)
    fl = floors(E, H * W, taps, C, 1, 4 * (f1.numel() + f2.numel() + coords.numel()), 4 * ours.numel())
    t_ours = timed(lambda: droid_backends.altcorr_forward(f1, f2, coords, r))
    t_theirs = timed(lambda: composition(f1, f2, coords, r), reps=5, warm=1)
    res["forward"] = dict(hip_ms=t_ours, composition_ms=t_theirs, composition_over_hip=t_theirs / t_ours,
                          agree=agree(ours[:, 0], theirs),
                          hip_peak_bytes=peak_bytes(lambda: droid_backends.altcorr_forward(f1, f2, coords, r)),
                          composition_peak_bytes=peak_bytes(lambda: composition(f1, f2, coords, r)), floors=fl,
                          fraction_of_floor=max(fl["fma_floor_ms"], fl["traffic_floor_ms"]) / t_ours)
    t_smooth = timed(lambda: droid_backends.altcorr_forward(f1, f2, smooth, r))
    res["forward_smooth_flow"] = dict(hip_ms=t_smooth, composition_over_hip=t_theirs / t_smooth,
                                      agree=agree(droid_backends.altcorr_forward(f1, f2, smooth, r)[0][:, 0],
                                                  composition(f1, f2, smooth, r)),
                                      fraction_of_floor=max(fl["fma_floor_ms"], fl["traffic_floor_ms"]) / t_smooth)
    del theirs

    # (c) the backward against autograd through the composition
    grad = torch.randn_like(ours)
    a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)

    def autograd_backward():
        out = composition(a1, a2, coords, r)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        grads = torch.autograd.grad(out, (a1, a2), grad[:, 0])
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), grads

    ts = sorted(autograd_backward()[0] for _ in range(5))
    g_theirs = autograd_backward()[1]
    g_ours = droid_backends.altcorr_backward(f1, f2, coords, grad, r)
    res["backward"] = dict(hip_ms=timed(lambda: droid_backends.altcorr_backward(f1, f2, coords, grad, r), reps=5,
                                        warm=1),
                           autograd_ms=ts[len(ts) // 2], agree_fmap1=agree(g_ours[0], g_theirs[0], tol=1e-2),
                           agree_fmap2=agree(g_ours[1], g_theirs[1], tol=1e-2),
                           note="autograd: the backward of the composition alone, its forward excluded")
    res["backward"]["autograd_over_hip"] = res["backward"]["autograd_ms"] / res["backward"]["hip_ms"]
    del g_theirs, g_ours, a1, a2, f1, f2, ours, grad

    # (b) the fused block on the fp16 buffer against the per-level call pattern
    fmaps = torch.randn(1, frames, C, H, W, device=dev, generator=g).half()
    ii = torch.arange(E, device=dev) % frames
    jj = (ii + 1 + torch.arange(E, device=dev) // frames) % frames
    block = AltCorrBlock(fmaps, num_levels=levels, radius=r)
    bc = coords.view(1, E, H, W, 2)
    ours = block(bc, ii, jj)
    theirs = call_pattern(block, bc, ii, jj)
    in_bytes = 2 * sum(p.numel() for p in block.pyramid) + 2 * block.pyramid[0].numel() * (levels - 1) + 4 * bc.numel()
    fl = floors(E, H * W, taps, C, levels, in_bytes, 4 * ours.numel())
    t_ours = timed(lambda: block(bc, ii, jj))
    t_theirs = timed(lambda: call_pattern(block, bc, ii, jj), reps=5, warm=1)
    res["block"] = dict(hip_ms=t_ours, call_pattern_ms=t_theirs, call_pattern_over_hip=t_theirs / t_ours,
                        identical=bool(torch.equal(ours, theirs)), agree=agree(ours, theirs),
                        hip_peak_bytes=peak_bytes(lambda: block(bc, ii, jj)),
                        call_pattern_peak_bytes=peak_bytes(lambda: call_pattern(block, bc, ii, jj)),
                        output_bytes=4 * ours.numel(), floors=fl,
                        fraction_of_floor=max(fl["fma_floor_ms"], fl["traffic_floor_ms"]) / t_ours)
    bs = smooth.view(1, E, H, W, 2)
    t_ours, t_theirs = timed(lambda: block(bs, ii, jj)), timed(lambda: call_pattern(block, bs, ii, jj), reps=5, warm=1)
    res["block_smooth_flow"] = dict(hip_ms=t_ours, call_pattern_ms=t_theirs, call_pattern_over_hip=t_theirs / t_ours,
                                    identical=bool(torch.equal(block(bs, ii, jj), call_pattern(block, bs, ii, jj))),
                                    fraction_of_floor=max(fl["fma_floor_ms"], fl["traffic_floor_ms"]) / t_ours)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
