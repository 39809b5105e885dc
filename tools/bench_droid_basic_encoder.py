#!/usr/bin/env python
"""wgsr.frontend.feature_encoder / context_encoder (csrc/droid_basic_encoder.hip:
14 convolution launches per call, for fnet one small statistics launch per raw
map besides) against what the tracker runs without them: the ``BasicEncoder``
module as a torch composition under autocast (``DroidNet.fnet`` on every
incoming frame, ``.cnet`` on every keyframe; motion_filter.py:39-48, 61-70).

The composition is this tool's own restatement of the module from its layer
table (stem 7 x 7 stride 2; three stages of two residual blocks with 32, 64 and
128 channels, the last two entered at stride 2 with a 1 x 1 stride-2 downsample
on the skip path; a 1 x 1 head; an instance norm or none after every
convolution but the head), with the caller's tanh / relu split for cnet.

Same GPU and build, 1 and 8 images of 384 x 512.

* ``*_call_us``  device time per call as the caller sees it: HIP events around
                 a batch of back-to-back calls (after warm-up), the median over
                 repeats with the smallest and largest (the spread), the two
                 forms alternating batch by batch.  The fused call runs on a
                 ``BasicEncoderWorkspace`` and an ``out`` buffer.
* ratio          torch / fused: above 1 means the project's call is faster.
* model          the FLOPs the kernels execute (whole tiles, the stem's K padded
                 to 160), the useful FLOPs, the bytes the launches have to move
                 (every map written once and read by its consumers, the packed
                 weights once), the floors at the fp16 MFMA peak and at the
                 measured HBM copy rate.
* difference     the largest difference from the autocast composition in units
                 of the float16 spacing at the composition's value (which is
                 tiny where that value is near zero) and of the spacing at the
                 output's rms, and its rms relative to the output's rms
                 (autocast rounds more often: after every norm, ReLU and sum).

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
DIMS = (32, 64, 128)


class Block(nn.Module):
    def __init__(self, c_in, c_out, norm, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(c_in, c_out, 3, stride, 1)
        self.conv2 = nn.Conv2d(c_out, c_out, 3, 1, 1)
        self.n1, self.n2 = norm(c_out), norm(c_out)
        self.downsample = nn.Sequential(nn.Conv2d(c_in, c_out, 1, stride), norm(c_out)) if stride > 1 else None

    def forward(self, x):
        y = torch.relu(self.n1(self.conv1(x)))
        y = torch.relu(self.n2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return torch.relu(x + y)


class Encoder(nn.Module):
    def __init__(self, out_dim, instance):
        super().__init__()
        norm = (lambda c: nn.InstanceNorm2d(c)) if instance else (lambda c: nn.Identity())
        self.conv1, self.n1 = nn.Conv2d(3, DIMS[0], 7, 2, 3), norm(DIMS[0])
        self.layer1 = nn.Sequential(Block(32, 32, norm, 1), Block(32, 32, norm, 1))
        self.layer2 = nn.Sequential(Block(32, 64, norm, 2), Block(64, 64, norm, 1))
        self.layer3 = nn.Sequential(Block(64, 128, norm, 2), Block(128, 128, norm, 1))
        self.conv2 = nn.Conv2d(DIMS[2], out_dim, 1)

    def forward(self, x):
        x = torch.relu(self.n1(self.conv1(x)))
        return self.conv2(self.layer3(self.layer2(self.layer1(x))))


def batch_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def compare(forms, calls, reps):
    for _ in range(3):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            times[k].append(batch_ms(f, calls))
    t = {}
    for k, v in times.items():
        v.sort()
        t[k] = dict(median=1e3 * v[len(v) // 2], min=1e3 * v[0], max=1e3 * v[-1])
    spread = max(v["max"] - v["min"] for v in t.values())
    diff = t["torch"]["median"] - t["fused"]["median"]
    return dict(torch_call_us=t["torch"], fused_call_us=t["fused"],
                torch_over_fused=t["torch"]["median"] / t["fused"]["median"], median_difference_us=diff,
                largest_spread_us=spread, fused_faster_by_more_than_the_spread=bool(diff > spread))


def model(n, H, W, out_dim, instance):
    """FLOPs and bytes of one call (see the module's text)"""
    sizes, image_bytes = [], 3 * H * W * 4
    for _ in range(3):
        H, W = (H + 1) // 2, (W + 1) // 2
        sizes.append((H, W))
    tiles = lambda s, ty: ((s[0] + ty - 1) // ty) * ((s[1] + 15) // 16) * 16 * ty  # noqa: E731  (pixels of whole tiles)
    px = lambda s: s[0] * s[1]  # noqa: E731
    # (output level, rows3, rows1, C_in, tile rows)
    launches = [(0, 32, 0, 32, 8)] * 4 + [(1, 64, 64, 32, 4)] + [(1, 64, 0, 64, 8)] * 3 + [(2, 128, 128, 64, 4)] + \
        [(2, 128, 0, 128, 8)] * 3 + [(2, 0, out_dim, 128, 8)]
    executed = 2 * tiles(sizes[0], 8) * 32 * 160
    useful = 2 * px(sizes[0]) * 32 * 147
    weights = 32 * 160
    # the image; every raw map is written once and read once (the statistics and their partial sums, a few hundred
    # KB for fnet, are left out)
    moved = image_bytes + 2 * 2 * px(sizes[0]) * 32
    for level, rows3, rows1, c_in, ty in launches:
        k = 9 * rows3 * c_in + rows1 * c_in
        executed += 2 * tiles(sizes[level], ty) * k
        useful += 2 * px(sizes[level]) * k
        weights += k
        moved += 2 * 2 * px(sizes[level]) * (rows3 + rows1)
    # the block outputs X0, X1, X3, X5: written once, read once
    moved += 2 * 2 * (2 * px(sizes[0]) * 32 + px(sizes[1]) * 64 + px(sizes[2]) * 128)
    executed, useful, moved = n * executed, n * useful, n * moved + 2 * weights
    return dict(executed_flops=executed, useful_flops=useful, moved_bytes=moved,
                mfma_floor_us=1e6 * executed / F16_MFMA_FLOPS, hbm_floor_us=1e6 * moved / HBM_BYTES_PER_S)


def ulps(a, b):
    """the largest |a - b| in units of the float16 spacing at |b|"""
    a, b = a.double(), b.double()
    spacing = torch.exp2(torch.floor(torch.log2(b.abs().clamp_min(2.0 ** -14))) - 10)
    return float(((a - b).abs() / spacing).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    from wgsr import frontend
    dev = torch.device("cuda:0")
    H, W = (48, 64) if args.small else (384, 512)
    counts = (1, 2) if args.small else (1, 8)
    res = {"device": torch.cuda.get_device_name(0),
           "problem": dict(images=f"{H}x{W}", counts=list(counts), calls_per_batch=args.calls, repeats=args.reps)}
    with torch.no_grad():
        for name, norm, out_dim in (("fnet", "instance", 128), ("cnet", "none", 256)):
            torch.manual_seed(31)
            net = Encoder(out_dim, norm == "instance").to(dev).eval()
            if norm == "none":
                net.conv2.weight.mul_(1.0 / 12)     # (without a norm the residual sums grow: keep tanh off saturation)
            params = frontend.BasicEncoder.from_state_dict(net.state_dict(), prefix="", norm=norm)
            f = frontend.feature_encoder if norm == "instance" else frontend.context_encoder
            for n in counts:
                g = torch.Generator(device=dev).manual_seed(n)
                images = torch.randn(n, 3, H, W, device=dev, generator=g)
                ws = frontend.BasicEncoderWorkspace(n, H, W, norm, dev)
                shape = (n, 128) + frontend.be_sizes(H, W)[2]
                out = tuple(torch.empty(shape, dtype=torch.float16, device=dev) for _ in range(out_dim // 128))

                def composition():
                    with torch.autocast("cuda", dtype=torch.float16):
                        x = net(images)
                        if norm == "none":
                            return x[:, :128].tanh(), x[:, 128:].relu()
                        return (x,)

                def fused():
                    return f(images, params, out=out[0] if norm == "instance" else out, workspace=ws)

                a = [t.float().clone() for t in composition()]
                fused()
                b = [t.float().clone() for t in out]
                r = compare({"torch": composition, "fused": fused}, args.calls, args.reps)
                r["difference_to_the_autocast_composition"] = dict(
                    largest_in_float16_ulps=[ulps(y, x) for x, y in zip(a, b)],
                    largest_in_ulps_at_the_output_rms=[ulps(y - x + x.pow(2).mean().sqrt(), x.pow(2).mean().sqrt())
                                                       for x, y in zip(a, b)],
                    rms_over_output_rms=[float((x - y).pow(2).mean().sqrt() / x.pow(2).mean().sqrt())
                                         for x, y in zip(a, b)])
                r["launches"] = dict(fused=14 + (13 if norm == "instance" else 0),
                                     of_which_statistics=13 if norm == "instance" else 0)
                r["model"] = model(n, H, W, out_dim, norm == "instance")
                res[f"{name}_{n}"] = r
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
