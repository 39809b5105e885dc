#!/usr/bin/env python
"""wgsr.frontend.CorrBlock (csrc/droid_corrvol.hip) on the MI355X against what
a user has without it: the reference's torch composition of the same class
(both maps / 4, ``torch.matmul``, three ``avg_pool2d``; ``torch.cat`` per level
to add edges, a boolean gather per level to drop them; per level a scaled copy
of the coordinates and one ``droid_backends.corr_index_forward``, then a
``torch.cat``), restated here as ``Composition``, on the same GPU.

Device time per call from HIP events -- the median of ``--reps`` windows after a
warm-up, each window ``inner`` calls long so that a short call is not a
measurement of the event pair -- and peak device memory above what was
allocated before the call (``torch.cuda.max_memory_allocated``).  At 48 x 64
maps, C = 128, fp16, r = 3, four levels:

* build1, build8    one edge, eight edges: ``CorrBlock(fmap1, fmap2)`` against
                    ``Composition(fmap1, fmap2)``; ``kernel_ms`` is the build
                    launch alone into a store that exists
* lookup75          one lookup of 75 edges
* add8_to_67        ``block.append`` against build + ``cat``
* drop8_of_75       ``block[mask]`` against the gather (``wall_ms``: host clock
                    around the call and a synchronise; the mask is read on the
                    host by both)
* motion_filter     build one edge, look it up once

``floors`` are derived from the shapes, not measured: the bytes a build must
store (one slot) and a lookup must move (the taps it reads, its output, the
coordinates) at the measured HBM copy rate, and the build's 2 (HW)^2 C flop at
the fp16 matrix peak.  Prints one JSON object; ``--out FILE`` also writes it.
``--small`` shrinks every problem (a quick check of the tool itself).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "wildgs-slam-blackwell_amd", "python"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_FP16_MFMA_FLOPS = 2.5e15  # dense, datasheet
HBM_BYTES_PER_S = 6.29e12      # measured float4 copy


class Composition:
    """The all-pairs pyramid as torch calls, in the reference's order of
    operations, over this project's ``corr_index_forward``."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=3):
        self.radius = radius
        b, n, c, h, w = fmap1.shape
        a1 = fmap1.reshape(b * n, c, h * w) / 4.0
        a2 = fmap2.reshape(b * n, c, h * w) / 4.0
        vol = torch.matmul(a1.transpose(1, 2), a2).reshape(b * n * h * w, 1, h, w)
        self.levels = []
        for i in range(num_levels):
            self.levels.append(vol.view(b * n, h, w, h >> i, w >> i))
            vol = F.avg_pool2d(vol, kernel_size=2, stride=2)

    def __call__(self, coords):
        return per_level_lookup(self.levels, coords, self.radius)

    def cat(self, other):
        self.levels = [torch.cat([a, b], dim=0) for a, b in zip(self.levels, other.levels)]
        return self

    def __getitem__(self, index):
        self.levels = [a[index] for a in self.levels]
        return self


def per_level_lookup(levels, coords, radius):
    import droid_backends
    b, n, h, w, _ = coords.shape
    planar = coords.permute(0, 1, 4, 2, 3).contiguous().view(b * n, 2, h, w)
    out = [droid_backends.corr_index_forward(level, planar / 2 ** i, radius)[0].view(b, n, -1, h, w)
           for i, level in enumerate(levels)]
    return torch.cat(out, dim=2)


def timed(fn, reps, inner=1, setup=None, warm=2):
    """(median device ms per call, median host ms per call incl. a synchronise)"""
    dev_ms, wall_ms = [], []
    for k in range(warm + reps):
        if setup is not None:
            setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warm:
            wall_ms.append(1e3 * (time.perf_counter() - t0) / inner)
            dev_ms.append(a.elapsed_time(b) / inner)
    dev_ms.sort()
    wall_ms.sort()
    return dev_ms[len(dev_ms) // 2], wall_ms[len(wall_ms) // 2]


def peak_bytes(fn, setup=None):
    if setup is not None:
        setup()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def row(ours, theirs, reps, inner=1, setup_ours=None, setup_theirs=None, floor_ms=None):
    o_dev, o_wall = timed(ours, reps, inner, setup_ours)
    t_dev, t_wall = timed(theirs, reps, inner, setup_theirs)
    r = dict(hip_ms=o_dev, composition_ms=t_dev, composition_over_hip=t_dev / o_dev if o_dev > 0 else None,
             hip_wall_ms=o_wall, composition_wall_ms=t_wall, hip_peak_bytes=peak_bytes(ours, setup_ours),
             composition_peak_bytes=peak_bytes(theirs, setup_theirs))
    if floor_ms is not None:
        r["floor_ms"] = floor_ms
        r["hip_over_floor"] = o_dev / floor_ms
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    from wgsr import frontend
    from wgsr.frontend import CorrBlock
    dev = torch.device("cuda:0")
    H, W, C, r, L, held, batch = (16, 24, 64, 3, 4, 9, 2) if args.small else (48, 64, 128, 3, 4, 75, 8)
    HW, rd2, taps = H * W, (2 * r + 1) ** 2, (2 * r + 2) ** 2
    g = torch.Generator(device=dev).manual_seed(4)
    f1 = torch.randn(1, held, C, H, W, device=dev, generator=g).half()
    f2 = torch.randn(1, held, C, H, W, device=dev, generator=g).half()
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev),
                          torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
    coords = (torch.stack([u, v], -1)[None, None] + 4 * torch.randn(1, held, H, W, 2, device=dev, generator=g)).contiguous()
    slot_bytes = 2 * frontend.corr_slot_layout(H, W, L)[1]
    res = {"device": torch.cuda.get_device_name(0),
           "problem": dict(maps=f"{H}x{W}", channels=C, radius=r, levels=L, held_edges=held, batch=batch)}
    build_floor = dict(stored_bytes_per_edge=slot_bytes, store_floor_ms_per_edge=1e3 * slot_bytes / HBM_BYTES_PER_S,
                       input_bytes_per_edge=4 * C * HW, flop_per_edge=2 * HW * HW * C,
                       mfma_floor_ms_per_edge=1e3 * 2 * HW * HW * C / PEAK_FP16_MFMA_FLOPS)
    lookup_bytes = held * (sum(HW * min(taps, (H >> i) * (W >> i)) for i in range(L)) * 2 + L * rd2 * HW * 2 + HW * 8)
    res["floors"] = dict(build=build_floor, lookup=dict(unique_bytes=lookup_bytes,
                                                        traffic_floor_ms=1e3 * lookup_bytes / HBM_BYTES_PER_S))
    per_edge_floor = max(build_floor["store_floor_ms_per_edge"], build_floor["mfma_floor_ms_per_edge"])

    # (a) build of 1 edge and of `batch` edges; the launch alone into a store that exists
    for n in (1, batch):
        a, b = f1[:, :n].contiguous(), f2[:, :n].contiguous()
        ours, theirs = CorrBlock(a, b, L, r), Composition(a, b, L, r)
        same = all(torch.equal(x, y) for x, y in zip(ours.corr_pyramid, theirs.levels))
        close = [float(((x.float() - y.float()).abs() <= 2 ** -9 * y.float().abs() + 1e-3).float().mean())
                 for x, y in zip(ours.corr_pyramid, theirs.levels)]
        store, slots = ours._store, ours._slots()
        a4, b4 = a[0], b[0]
        k_ms, _ = timed(lambda: frontend.corr_build(a4, b4, store, slots, L), args.reps, inner=20)
        del ours, theirs
        res[f"build{n}"] = dict(row(lambda: CorrBlock(a, b, L, r), lambda: Composition(a, b, L, r), args.reps, inner=5,
                                    floor_ms=n * per_edge_floor),
                                kernel_ms=k_ms, kernel_over_floor=k_ms / (n * per_edge_floor),
                                pyramid_identical=same, pyramid_agree=close)

    # (b) one lookup at `held` edges
    block = CorrBlock(f1, f2, L, r, capacity=held + batch)
    comp = Composition(f1, f2, L, r)
    res["lookup%d" % held] = dict(row(lambda: block(coords), lambda: comp(coords), args.reps, inner=5,
                                      floor_ms=res["floors"]["lookup"]["traffic_floor_ms"]),
                                  identical_on_own_pyramid=bool(torch.equal(
                                      block(coords), per_level_lookup(block.corr_pyramid, coords, r))))

    # (c) adding `batch` edges to held - batch, (d) dropping `batch` of held
    base = list(comp.levels)
    keep = held - batch
    n1, n2 = f1[:, keep:].contiguous(), f2[:, keep:].contiguous()
    mask = torch.ones(held, dtype=torch.bool, device=dev)
    mask[torch.arange(batch, device=dev) * (held // batch) + 1] = False

    def ours_to(n):
        def setup():
            if len(block) > n:
                block[:n]
            elif len(block) < n:
                block.append(f1[:, len(block):n].contiguous(), f2[:, len(block):n].contiguous())
        return setup

    def theirs_to(n):
        def setup():
            comp.levels = [a[:n] for a in base]
        return setup

    res[f"add{batch}_to_{keep}"] = row(lambda: block.append(n1, n2), lambda: comp.cat(Composition(n1, n2, L, r)),
                                       args.reps, setup_ours=ours_to(keep), setup_theirs=theirs_to(keep),
                                       floor_ms=batch * per_edge_floor)
    res[f"drop{batch}_of_{held}"] = row(lambda: block[mask], lambda: comp[mask], args.reps, setup_ours=ours_to(held),
                                        setup_theirs=theirs_to(held))
    del block, comp, base

    # (e) the motion filter: build one edge, look it up once
    a, b, c1 = f1[:, :1].contiguous(), f2[:, :1].contiguous(), coords[:, :1].contiguous()
    res["motion_filter"] = row(lambda: CorrBlock(a, b, L, r)(c1), lambda: Composition(a, b, L, r)(c1), args.reps,
                               inner=5)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
