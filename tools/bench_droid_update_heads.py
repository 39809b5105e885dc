#!/usr/bin/env python
"""wgsr.frontend.update_heads / graph_agg (csrc/droid_conv3x3.hip, three launches
each) against the torch composition the tracker runs per update iteration --
the same ``Conv2d``s under autocast (``UpdateModule.delta`` / ``.weight`` with
the permute of droid_net.py:144-145; ``GraphAgg``'s conv1, an ``index_add_``
mean, conv2 and the eta head) -- on the same GPU and build, at the tracker's
shape (48 x 64 maps) for 24, 48 and 96 edges over 12 frames.

* ``*_call_us``  device time per call as the caller sees it: HIP events around
                 a batch of back-to-back calls (after warm-up), the median over
                 repeats, the fused and composed forms alternating batch by
                 batch.
* ratios         composed / fused: above 1 means the project's call is faster.
* model          the FLOPs the kernels execute (padded head rows included) and
                 the useful ones, the bytes each launch has to move, the floor
                 at the fp16 MFMA peak and the measured HBM copy rate, and
                 ``mfma_fraction``: executed FLOPs / call time / the MFMA peak.
* ``kernel_us``  the kernel's own time, when ``--kernel-stats CSV`` names the
                 kernel statistics of a ``rocprofv3 --kernel-trace --stats`` run
                 of this tool (a run of its own); otherwise "not measured".

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
from torch import nn  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy
F16_MFMA_FLOPS = 2.5e15     # dense fp16 MFMA peak
K = 9 * 128


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
    out = []
    for r in csv.DictReader(open(path)):
        if "k_conv3x3" in r["Name"]:
            out.append(dict(name=r["Name"], avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3,
                            max_us=float(r["MaxNs"]) / 1e3, calls=int(r["Calls"])))
    return out


def conv(c_out):
    return nn.Conv2d(128, c_out, kernel_size=3, padding=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--kernel-stats", help="kernel stats CSV of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--edges", help="edge counts, comma-separated (default 24,48,96)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    from wgsr import frontend
    dev = torch.device("cuda:0")
    ht, wd = (6, 8) if args.small else (48, 64)
    counts = (4, 6) if args.small else (24, 48, 96)
    frames = 3 if args.small else 12
    if args.edges:
        counts = tuple(int(v) for v in args.edges.split(","))
    torch.manual_seed(11)
    delta = nn.Sequential(conv(128), nn.ReLU(inplace=True), conv(2)).to(dev)
    weight = nn.Sequential(conv(128), nn.ReLU(inplace=True), conv(2), nn.Sigmoid()).to(dev)
    conv1, conv2, eta = conv(128).to(dev), conv(128).to(dev), nn.Sequential(conv(1), nn.Softplus()).to(dev)
    sd = {}
    for name, m in (("delta.0", delta[0]), ("delta.2", delta[2]), ("weight.0", weight[0]), ("weight.2", weight[2]),
                    ("agg.conv1", conv1), ("agg.conv2", conv2), ("agg.eta.0", eta[0])):
        sd[name + ".weight"], sd[name + ".bias"] = m.weight, m.bias
    params = frontend.UpdateHeads.from_state_dict(sd, prefix="")
    res = {"device": torch.cuda.get_device_name(0),
           "problem": dict(maps=f"{ht}x{wd}", frames=frames, edges=list(counts), calls_per_batch=args.calls,
                           repeats=args.reps),
           "kernel_us": kernel_times(args.kernel_stats) if args.kernel_stats else "not measured"}
    with torch.no_grad():
        for n in counts:
            g = torch.Generator(device=dev).manual_seed(n)
            net = torch.randn(n, 128, ht, wd, device=dev, generator=g).half()
            ii = torch.randint(0, frames, (n,), device=dev, generator=g)
            ii[:frames] = torch.arange(frames, device=dev)   # every frame is the source of an edge
            ix = torch.unique(ii, sorted=True, return_inverse=True)[1].contiguous()
            G = frames
            count = torch.zeros(G, device=dev).index_add_(0, ix, torch.ones(n, device=dev)).clamp(min=1)

            def torch_heads():
                with torch.autocast("cuda", dtype=torch.float16):
                    d, w = delta(net), weight(net)
                return d.permute(0, 2, 3, 1).contiguous(), w.permute(0, 2, 3, 1).contiguous()

            def torch_agg():
                with torch.autocast("cuda", dtype=torch.float16):
                    x = torch.relu(conv1(net))
                    mean = torch.zeros(G, 128, ht, wd, dtype=x.dtype, device=dev).index_add_(0, ix, x)
                    mean = mean / count.view(G, 1, 1, 1).to(x.dtype)
                    feat = torch.relu(conv2(mean))
                    return 0.01 * eta(feat)[:, 0], feat

            forms = {
                "heads_composed": torch_heads,
                "heads_fused": lambda: frontend.update_heads(net, params),
                "agg_composed": torch_agg,
                "agg_fused": lambda: frontend.graph_agg(net, None, params, ix=ix, num_groups=G, check=False),
            }
            outs = {k: f() for k, f in forms.items()}
            torch.cuda.synchronize()
            diff = {"delta": float((outs["heads_fused"][0] - outs["heads_composed"][0].float()).abs().max()),
                    "weight": float((outs["heads_fused"][1] - outs["heads_composed"][1].float()).abs().max()),
                    "eta": float((outs["agg_fused"][0] - outs["agg_composed"][0].float()).abs().max()),
                    "feat": float((outs["agg_fused"][1].float() - outs["agg_composed"][1].float()).abs().max())}
            t = alternate(forms, args.calls, args.reps)
            px, gpx = n * ht * wd, G * ht * wd
            heads_flops, heads_useful = 2 * px * K * (256 + 16 + 16), 2 * px * K * (256 + 2 + 2)
            agg_flops, agg_useful = 2 * K * (px * 128 + gpx * (128 + 16)), 2 * K * (px * 128 + gpx * (128 + 1))
            # net read, hidden written and read once, the fp32 outputs; the packed weights once
            heads_bytes = px * (128 * 2 + 2 * 256 * 2 + 2 * 2 * 4) + K * (256 + 32) * 2
            # net read, the mean written and read, feat written and read, eta
            agg_bytes = px * 128 * 2 + gpx * (4 * 128 * 2 + 4) + K * (256 + 16) * 2
            rec = {k + "_call_us": v for k, v in t.items()}
            rec.update(
                heads_composed_over_fused=t["heads_composed"]["median"] / t["heads_fused"]["median"],
                agg_composed_over_fused=t["agg_composed"]["median"] / t["agg_fused"]["median"],
                max_abs_difference_to_composed=diff,
                heads_model=dict(executed_flops=heads_flops, useful_flops=heads_useful, unique_bytes=heads_bytes,
                                 floor_us=1e6 * max(heads_flops / F16_MFMA_FLOPS, heads_bytes / HBM_BYTES_PER_S),
                                 mfma_fraction=heads_flops / (1e-6 * t["heads_fused"]["median"]) / F16_MFMA_FLOPS),
                agg_model=dict(executed_flops=agg_flops, useful_flops=agg_useful, unique_bytes=agg_bytes,
                               floor_us=1e6 * max(agg_flops / F16_MFMA_FLOPS, agg_bytes / HBM_BYTES_PER_S),
                               mfma_fraction=agg_flops / (1e-6 * t["agg_fused"]["median"]) / F16_MFMA_FLOPS))
            res[f"edges_{n}"] = rec
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
