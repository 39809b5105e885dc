#!/usr/bin/env python
"""wgsr.frontend.conv_gru (csrc/droid_gru.hip, four launches) against the torch
composition of the same formulas as the tracker runs them per update iteration
-- ``Conv2d``s under autocast, both ``torch.cat``s included:

    glo = mean over pixels of sigmoid(w(net)) * net
    z = sigmoid(convz(cat[net, inp, corr, flow]) + convz_glo(glo)), r likewise
    q = tanh(convq(cat[r * net, inp, corr, flow]) + convq_glo(glo))
    net' = (1 - z) net + z q

on the same GPU and build, at the tracker's shape (48 x 64 maps) for 24, 48 and
96 edges.

* ``*_call_us``  device time per call as the caller sees it: HIP events around
                 a batch of back-to-back calls (after warm-up), the median over
                 repeats with the smallest and largest (the spread), the fused
                 and composed forms alternating batch by batch.
* ratio          composed / fused: above 1 means the project's call is faster.
* model          the FLOPs the kernels execute, the bytes the launches have
                 to move (every activation once, z and rnet written and
                 read, the packed weights once), the weight bytes the
                 workgroups read from L2 by count, the floor at the fp16 MFMA
                 peak and the measured HBM copy rate, and ``mfma_fraction``:
                 executed FLOPs / call time / the MFMA peak.
* ``kernel_us``  the kernels' own times, when ``--kernel-stats CSV`` names the
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
CIN = 448
K = 9 * CIN
NAMES = ("convz", "convr", "convq", "w", "convz_glo", "convr_glo", "convq_glo")


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
        if "k_gru" in r["Name"]:
            out.append(dict(name=r["Name"], avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3,
                            max_us=float(r["MaxNs"]) / 1e3, calls=int(r["Calls"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--kernel-stats", help="kernel stats CSV of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--edges", help="edge counts, comma-separated (default 24,48,96)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    from wgsr import frontend
    dev = torch.device("cuda:0")
    ht, wd = (6, 8) if args.small else (48, 64)
    counts = (4, 6) if args.small else (24, 48, 96)
    if args.edges:
        counts = tuple(int(v) for v in args.edges.split(","))
    torch.manual_seed(13)
    m = {k: (nn.Conv2d(CIN, 128, 3, padding=1) if k in NAMES[:3] else nn.Conv2d(128, 128, 1)).to(dev) for k in NAMES}
    sd = {}
    for name, conv in m.items():
        sd[name + ".weight"], sd[name + ".bias"] = conv.weight, conv.bias
    params = frontend.UpdateGRU.from_state_dict(sd, prefix="")
    res = {"device": torch.cuda.get_device_name(0),
           "problem": dict(maps=f"{ht}x{wd}", edges=list(counts), calls_per_batch=args.calls, repeats=args.reps),
           "kernel_us": kernel_times(args.kernel_stats) if args.kernel_stats else "not measured"}
    with torch.no_grad():
        for n in counts:
            g = torch.Generator(device=dev).manual_seed(n)
            net, inp, corr = (torch.randn(n, 128, ht, wd, device=dev, generator=g).half() for _ in range(3))
            flow = torch.randn(n, 64, ht, wd, device=dev, generator=g).half()
            out = torch.empty_like(net)
            scratch = (torch.empty(n, 384, device=dev), torch.empty_like(net), torch.empty_like(net),
                       torch.empty(n, (ht * wd + 127) // 128, 128, device=dev))

            def composed():
                with torch.autocast("cuda", dtype=torch.float16):
                    x = torch.cat([inp, corr, flow], dim=1)
                    net_x = torch.cat([net, x], dim=1)
                    glo = torch.sigmoid(m["w"](net)) * net
                    glo = glo.view(n, 128, ht * wd).mean(dim=-1, keepdim=True).view(n, 128, 1, 1)
                    z = torch.sigmoid(m["convz"](net_x) + m["convz_glo"](glo))
                    r = torch.sigmoid(m["convr"](net_x) + m["convr_glo"](glo))
                    q = torch.tanh(m["convq"](torch.cat([r * net, x], dim=1)) + m["convq_glo"](glo))
                    return (1 - z) * net + z * q

            forms = {"composed": composed,
                     "fused": lambda: frontend.conv_gru(net, inp, corr, flow, params, check=False, out=out,
                                                        scratch=scratch)}
            outs = {k: f().float().clone() for k, f in forms.items()}
            torch.cuda.synchronize()
            diff = float((outs["fused"] - outs["composed"]).abs().max())
            t = alternate(forms, args.calls, args.reps)
            px = n * ht * wd
            tiles = n * ((ht + 7) // 8) * ((wd + 15) // 16)
            flops = 2 * px * (K * 384 + 128 * 128) + 2 * n * 384 * 128
            # net read by all three launches, inp / corr / flow by two, z and rnet written and read, net' written,
            # gbias; the packed weights once
            unique = px * 2 * (3 * 128 + 2 * 320 + 2 * 2 * 128 + 128) + n * 384 * 4 * 3 + (K * 384 + 4 * 128 * 128) * 2
            # every workgroup of a convolution launch reads its 128 rows of packed weights: 3 passes per tile
            l2_weights = tiles * 3 * 128 * K * 2
            spread = max(v["max"] - v["min"] for v in t.values())
            res[f"edges_{n}"] = dict(
                composed_call_us=t["composed"], fused_call_us=t["fused"],
                composed_over_fused=t["composed"]["median"] / t["fused"]["median"],
                median_difference_us=t["composed"]["median"] - t["fused"]["median"], largest_spread_us=spread,
                max_abs_difference_to_composed=diff,
                model=dict(executed_flops=flops, unique_bytes=unique, l2_weight_bytes_by_count=l2_weights,
                           floor_us=1e6 * max(flops / F16_MFMA_FLOPS, unique / HBM_BYTES_PER_S),
                           mfma_fraction=flops / (1e-6 * t["fused"]["median"]) / F16_MFMA_FLOPS))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
