#!/usr/bin/env python
"""wgsr.frontend.upsample / upsample_from_features (csrc/droid_upsample.hip, one
launch each) against the torch composition the tracker runs per update
iteration -- the mask head (a 1 x 1 convolution 128 -> 576 under autocast), the
reference's ``cvx_upsample`` operation sequence (softmax, unfold, multiply, sum,
permute + contiguous) and the indexed gather / assign on the video buffers --
on the same GPU and build, at the tracker's shape (48 x 64 maps, C = 128) for
4, 12 and 24 frames.

* ``*_call_us``  device time per call as the caller sees it: HIP events around
                 a batch of back-to-back calls (after warm-up), the median over
                 repeats, the forms alternating batch by batch.  For a
                 one-launch form this is bounded below by how fast Python can
                 enqueue it, so it is a call time, not a kernel time.
                   composed        head + cvx_upsample + assign, all torch
                   composed_tail   cvx_upsample + assign (the mask given)
                   head_upsample   torch head, then frontend.upsample
                   upsample        frontend.upsample (the mask given)
                   fused           frontend.upsample_from_features
* ratios         composed / head_upsample, composed / fused, composed_tail /
                 upsample: above 1 means the project's call is faster.
* ``kernel_us``  the kernels' own time, when ``--kernel-stats CSV`` names the
                 kernel statistics of a ``rocprofv3 --kernel-trace --stats`` run
                 of this tool (a run of its own: tracing slows the host);
                 otherwise "not measured".  ``*_floor_us`` are the byte / flop
                 models of DESIGN.md at the measured HBM copy rate and the MFMA
                 peak.

Prints one JSON object; ``--out FILE`` also writes it there.  ``--small``
shrinks the problem (a quick check of the tool itself).
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "wildgs-slam-blackwell_amd", "python"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy
F16_MFMA_FLOPS = 2.5e15     # dense fp16 MFMA peak


def torch_cvx_upsample(data, mask):
    """the reference's operation sequence for [n, ht, wd, dim] data"""
    n, ht, wd, dim = data.shape
    w = torch.softmax(mask.view(n, 1, 9, 8, 8, ht, wd), dim=2)
    nb = F.unfold(data.permute(0, 3, 1, 2).contiguous(), kernel_size=(3, 3), padding=(1, 1))
    up = torch.sum(w * nb.view(n, dim, 9, 1, 1, ht, wd), dim=2)
    return up.permute(0, 4, 2, 5, 3, 1).contiguous().reshape(n, 8 * ht, 8 * wd, dim)


def batch_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(forms, calls, reps):
    for _ in range(3):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            times[k].append(batch_ms(f, calls))
    out = {}
    for k, t in times.items():
        t.sort()
        out[k] = dict(median=1e3 * t[len(t) // 2], min=1e3 * t[0], max=1e3 * t[-1])
    return out


def kernel_times(path):
    """{kernel: [rows]} of the two kernels from a rocprofv3 kernel stats CSV (all frame counts pooled)"""
    out = {}
    for r in csv.DictReader(open(path)):
        for name in ("k_cvx_upsample", "k_upmask_upsample"):
            if name in r["Name"]:
                out.setdefault(name, []).append(dict(avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3,
                                                     max_us=float(r["MaxNs"]) / 1e3, calls=int(r["Calls"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--kernel-stats", help="kernel stats CSV of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--frames", help="frame counts, comma-separated (default 4,12,24); one count for a profiled run, "
                                     "whose kernel statistics are per kernel name")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    from wgsr import frontend
    dev = torch.device("cuda:0")
    ht, wd, C = (6, 8, 32) if args.small else (48, 64, 128)
    counts = (2, 3) if args.small else (4, 12, 24)
    if args.frames:
        counts = tuple(int(v) for v in args.frames.split(","))
    torch.manual_seed(11)
    head = torch.nn.Conv2d(C, 576, kernel_size=1).to(dev)
    res = {"device": torch.cuda.get_device_name(0),
           "problem": dict(maps=f"{ht}x{wd}", C=C, frames=list(counts), calls_per_batch=args.calls, repeats=args.reps),
           "kernel_us": kernel_times(args.kernel_stats) if args.kernel_stats else "not measured"}
    with torch.no_grad():
        for n in counts:
            num = 2 * n
            g = torch.Generator(device=dev).manual_seed(n)
            disps = 0.1 + torch.rand(num, ht, wd, device=dev, generator=g)
            ix = torch.randperm(num, device=dev, generator=g)[:n].contiguous()
            feat = torch.randn(n, C, ht, wd, device=dev, generator=g).half()
            ups = {k: torch.zeros(num, 8 * ht, 8 * wd, device=dev) for k in ("composed", "head_upsample", "fused")}

            def torch_head():
                with torch.autocast("cuda", dtype=torch.float16):
                    return head(feat)

            def assign(up, mask):  # DepthVideo.upsample, as FactorGraph.update calls it (autocast off)
                up[ix] = torch_cvx_upsample(disps[ix].unsqueeze(-1), mask).squeeze(-1)

            mask = torch_head()
            assert mask.dtype == torch.float16
            forms = {
                "composed": lambda: assign(ups["composed"], torch_head()),
                "composed_tail": lambda: assign(ups["composed"], mask),
                "head_upsample": lambda: frontend.upsample(disps, ups["head_upsample"], ix, torch_head(), check=False),
                "upsample": lambda: frontend.upsample(disps, ups["head_upsample"], ix, mask, check=False),
                "fused": lambda: frontend.upsample_from_features(disps, ups["fused"], ix, feat, head.weight, head.bias,
                                                                 check=False),
            }
            for f in forms.values():
                f()
            torch.cuda.synchronize()
            # the reference's update path rounds its softmax weights to float16: agreement to about 2^-11
            diff = {k: float((ups[k] - ups["composed"]).abs().max()) for k in ("head_upsample", "fused")}
            t = alternate(forms, args.calls, args.reps)
            px = n * ht * wd
            mask_bytes, out_bytes = px * 576 * 2, px * 64 * 4
            rec = {k + "_call_us": v for k, v in t.items()}
            rec.update(
                composed_over_head_upsample=t["composed"]["median"] / t["head_upsample"]["median"],
                composed_over_fused=t["composed"]["median"] / t["fused"]["median"],
                composed_tail_over_upsample=t["composed_tail"]["median"] / t["upsample"]["median"],
                max_abs_difference_to_composed=diff,
                upsample_unique_bytes=mask_bytes + out_bytes + px * 4,
                upsample_floor_us=1e6 * (mask_bytes + out_bytes + px * 4) / HBM_BYTES_PER_S,
                fused_unique_bytes=px * C * 2 + out_bytes + px * 4 + 576 * C * 2,
                fused_flops=2 * px * 576 * C,
                fused_floor_us=1e6 * max((px * C * 2 + out_bytes + px * 4 + 576 * C * 2) / HBM_BYTES_PER_S,
                                         2 * px * 576 * C / F16_MFMA_FLOPS))
            res[f"frames_{n}"] = rec
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
