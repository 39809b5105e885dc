#!/usr/bin/env python
"""wgsr.frontend.corr_encoder / flow_encoder (csrc/droid_encoders.hip, one launch
each) and wgsr.frontend.update_operator (the whole ``UpdateModule.forward``)
against what the tracker runs per update iteration without them:

* ``encoders``  the two fused calls against the torch composition of the same
                ``Conv2d``s and ReLUs under autocast, fed the float16 ``corr``
                and the float32 ``motn`` (``UpdateModule.corr_encoder`` /
                ``.flow_encoder``, droid_net.py:88-100, 136-137);
* ``operator``  ``update_operator`` against those torch encoders followed by the
                fused ``conv_gru``, ``update_heads`` and ``graph_agg``: the state
                before the encoders were fused.

Same GPU and build, the tracker's shape (48 x 64 maps) for 24, 48 and 96 edges
of 12 frames.

* ``*_call_us``  device time per call as the caller sees it: HIP events around
                 a batch of back-to-back calls (after warm-up), the median over
                 repeats with the smallest and largest (the spread), the two
                 forms alternating batch by batch.
* ratio          torch / fused: above 1 means the project's call is faster.
* model          (encoders) the FLOPs the kernels execute -- the first layers on
                 the 12 x 16 columns of every tile's halo, K padded to 224 --, the
                 bytes the launches have to move (inputs, outputs, the packed
                 weights once), the floor at the fp16 MFMA peak and the measured
                 HBM copy rate, and ``mfma_fraction``: executed FLOPs / call time
                 / the MFMA peak.

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
from torch import nn  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy
F16_MFMA_FLOPS = 2.5e15     # dense fp16 MFMA peak
FRAMES = 12


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


def compare(forms, calls, reps):
    t = alternate(forms, calls, reps)
    spread = max(v["max"] - v["min"] for v in t.values())
    diff = t["torch"]["median"] - t["fused"]["median"]
    return t, dict(torch_call_us=t["torch"], fused_call_us=t["fused"],
                   torch_over_fused=t["torch"]["median"] / t["fused"]["median"], median_difference_us=diff,
                   largest_spread_us=spread, fused_faster_by_more_than_the_spread=bool(diff > spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
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
    torch.manual_seed(17)
    corr_enc = nn.Sequential(nn.Conv2d(196, 128, 1), nn.ReLU(inplace=True), nn.Conv2d(128, 128, 3, padding=1),
                             nn.ReLU(inplace=True)).to(dev)
    flow_enc = nn.Sequential(nn.Conv2d(4, 128, 7, padding=3), nn.ReLU(inplace=True), nn.Conv2d(128, 64, 3, padding=1),
                             nn.ReLU(inplace=True)).to(dev)
    sd = {}
    for prefix, seq in (("corr_encoder", corr_enc), ("flow_encoder", flow_enc)):
        for k in (0, 2):
            sd[f"{prefix}.{k}.weight"], sd[f"{prefix}.{k}.bias"] = seq[k].weight, seq[k].bias
    convs = {k: nn.Conv2d(448, 128, 3, padding=1) for k in ("gru.convz", "gru.convr", "gru.convq")}
    convs.update({k: nn.Conv2d(128, 128, 1) for k in ("gru.w", "gru.convz_glo", "gru.convr_glo", "gru.convq_glo")})
    convs.update({k: nn.Conv2d(128, c, 3, padding=1) for k, c in (
        ("delta.0", 128), ("delta.2", 2), ("weight.0", 128), ("weight.2", 2), ("agg.conv1", 128), ("agg.conv2", 128),
        ("agg.eta.0", 1))})
    for name, conv in convs.items():
        conv.to(dev)
        sd[name + ".weight"], sd[name + ".bias"] = conv.weight, conv.bias
    params = frontend.UpdateOperator.from_state_dict(sd, prefix="")
    res = {"device": torch.cuda.get_device_name(0),
           "problem": dict(maps=f"{ht}x{wd}", edges=list(counts), frames=FRAMES, calls_per_batch=args.calls,
                           repeats=args.reps)}
    with torch.no_grad():
        for n in counts:
            g = torch.Generator(device=dev).manual_seed(n)
            net, inp = (torch.randn(n, 128, ht, wd, device=dev, generator=g).half() for _ in range(2))
            corr = torch.randn(n, 196, ht, wd, device=dev, generator=g).half()
            motn = (128 * torch.rand(n, 4, ht, wd, device=dev, generator=g) - 64).clamp(-64, 64)
            G = min(FRAMES, n)
            ix = torch.arange(n, device=dev) % G
            enc_out = (torch.empty(n, 128, ht, wd, dtype=torch.float16, device=dev),
                       torch.empty(n, 64, ht, wd, dtype=torch.float16, device=dev))
            op_out = (torch.empty_like(net), torch.empty(n, ht, wd, 2, device=dev), torch.empty(n, ht, wd, 2, device=dev),
                      torch.empty(G, ht, wd, device=dev), torch.empty(G, 128, ht, wd, dtype=torch.float16, device=dev))

            def torch_encoders():
                with torch.autocast("cuda", dtype=torch.float16):
                    return corr_enc(corr), flow_enc(motn)

            def fused_encoders():
                return (frontend.corr_encoder(corr, params.encoders, out=enc_out[0]),
                        frontend.flow_encoder(motn, params.encoders, out=enc_out[1]))

            def parent_operator():
                c, f = torch_encoders()
                new = frontend.conv_gru(net, inp, c, f, params.gru, check=False, out=op_out[0])
                frontend.update_heads(new, params.heads, out=op_out[1:3])
                frontend.graph_agg(new, None, params.heads, ix=ix, num_groups=G, check=False, out=op_out[3:])
                return op_out

            def fused_operator():
                return frontend.update_operator(net, inp, corr, motn, ix, params=params, num_groups=G, check=False,
                                                out=op_out)

            a, b = [t.float().clone() for t in torch_encoders()], [t.float().clone() for t in fused_encoders()]
            enc_diff = [float((x - y).abs().max()) for x, y in zip(a, b)]
            a = [t.float().clone() for t in parent_operator()]
            b = [t.float().clone() for t in fused_operator()]
            op_diff = [float((x - y).abs().max()) for x, y in zip(a, b)]
            torch.cuda.synchronize()
            _, enc = compare({"torch": torch_encoders, "fused": fused_encoders}, args.calls, args.reps)
            _, op = compare({"torch": parent_operator, "fused": fused_operator}, args.calls, args.reps)
            px = n * ht * wd
            tiles = n * ((ht + 7) // 8) * ((wd + 15) // 16)
            # per tile: both first layers 128 rows x 192 columns x K = 224; the second layers 128 (64) rows x 128
            # pixels x K = 1152
            flops = tiles * 2 * (2 * 128 * 192 * 224 + (128 + 64) * 128 * 1152)
            useful = px * 2 * (2 * 196 * 128 + (128 + 64) * 1152)
            unique = px * (196 * 2 + 4 * 4 + (128 + 64) * 2) + (2 * 128 * 224 + (128 + 64) * 1152) * 2
            enc["max_abs_difference_to_torch"] = dict(corr=enc_diff[0], flow=enc_diff[1])
            enc["model"] = dict(executed_flops=flops, useful_flops=useful, unique_bytes=unique,
                                floor_us=1e6 * max(flops / F16_MFMA_FLOPS, unique / HBM_BYTES_PER_S),
                                mfma_fraction=flops / (1e-6 * enc["fused_call_us"]["median"]) / F16_MFMA_FLOPS)
            op["max_abs_difference_to_torch_encoders"] = dict(zip(("net", "delta", "weight", "eta", "feat"), op_diff))
            res[f"edges_{n}"] = dict(encoders=enc, operator=op)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
