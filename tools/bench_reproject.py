#!/usr/bin/env python
"""wgsr.frontend.reproject (csrc/lie.hip k_reproject, one launch) against the
same result composed through the ``lietorch`` drop-in's generic operations (the
reference's projective_transform pattern), on the same GPU and build.

At the tracker's shape, 96 edges over 24 frames of 48 x 64, with and without
Jacobians:

* ``call_us``    device time per call as the caller sees it: HIP events around
                 a batch of back-to-back calls (after warm-up), the median over
                 repeats, fused and composed batches alternating.  For the
                 fused call this is bounded below by how fast Python can
                 enqueue it, so it is a call time, not a kernel time.
* ``device_ops`` what each form puts on the stream per call: the aten
                 operations dispatched (views and allocations excluded) plus
                 the group-kernel launches; 1 for the fused call.  Counted on
                 the host, not from a kernel trace.
* ``kernel_us``  k_reproject's own time, when ``--kernel-stats CSV`` names the
                 kernel statistics of a ``rocprofv3 --kernel-trace --stats`` run
                 of this tool (a run of its own: tracing slows the host);
                 otherwise "not measured".  ``fraction_of_byte_model`` =
                 unique bytes (n ht wd (4 + 12), + 104 with Jacobians) at the
                 measured HBM copy rate, over that kernel time.

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
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

HBM_BYTES_PER_S = 6.29e12   # measured float4 copy
MIN_DEPTH = 0.2
NO_LAUNCH = {"view", "unbind", "select", "slice", "expand", "unsqueeze", "squeeze", "alias", "empty", "empty_like",
             "empty_strided", "new_empty", "as_strided", "detach", "permute", "transpose", "reshape", "_unsafe_view",
             "t", "_reshape_alias", "lift_fresh"}  # aten operations that put nothing on the stream


def composed(poses, disps, intrinsics, ii, jj, jacobian, return_depth=False):
    """projective_transform's steps, one group operation or torch expression each"""
    from lietorch import SE3
    ht, wd = disps.shape[1:]
    dev = poses.device
    G = SE3(poses[None])
    Gij = G[:, jj] * G[:, ii].inv()
    Gij.data[:, ii == jj] = torch.tensor([-0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], device=dev)
    Ki, Kj = intrinsics[ii][None, :, None, None], intrinsics[jj][None, :, None, None]
    v, u = torch.meshgrid(torch.arange(ht, device=dev).float(), torch.arange(wd, device=dev).float(), indexing="ij")
    d = disps[ii][None]
    one = torch.ones_like(d)
    X0 = torch.stack([(u - Ki[..., 2]) / Ki[..., 0], (v - Ki[..., 3]) / Ki[..., 1], one, d], dim=-1)
    X1 = Gij[:, :, None, None] * X0
    X, Y, Z, D = X1.unbind(-1)
    fx, fy, cx, cy = Kj.unbind(-1)
    iz = 1.0 / torch.where(Z < 0.5 * MIN_DEPTH, one, Z)
    cs = [fx * (X * iz) + cx, fy * (Y * iz) + cy] + ([D * iz] if return_depth else [])
    coords = torch.stack(cs, -1)
    valid = ((Z > MIN_DEPTH) & (X0[..., 2] > MIN_DEPTH)).float()[..., None]
    if not jacobian:
        return coords, valid
    o = torch.zeros_like(d)
    Jp = torch.stack([fx * iz, o, -fx * X * iz * iz, o, o, fy * iz, -fy * Y * iz * iz, o], -1).view(d.shape + (2, 4))
    Ja = torch.stack([D, o, o, o, Z, -Y, o, D, o, -Z, o, X, o, o, D, Y, -X, o, o, o, o, o, o, o],
                     -1).view(d.shape + (4, 6))
    Jj = Jp @ Ja
    Ji = -Gij[:, :, None, None, None].adjT(Jj)
    e4 = torch.zeros_like(X0)
    e4[..., 3] = 1.0
    Jz = Jp @ (Gij[:, :, None, None] * e4)[..., None]
    return coords, valid, (Ji, Jj, Jz)


class OpCounter(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func._schema.name.split("::")[-1] not in NO_LAUNCH:
            self.n += 1
        return func(*args, **(kwargs or {}))


def count_device_ops(fn):
    from wgsr import _lib
    L = _lib.load()
    real = L.wgsr_lie_se3
    launches = [0]

    class Counting:  # the ctypes entry, counted
        def __call__(self, *a):
            launches[0] += 1
            return real(*a)

    L.wgsr_lie_se3 = Counting()
    try:
        with OpCounter() as c:
            fn()
    finally:
        L.wgsr_lie_se3 = real
    return c.n + launches[0], launches[0]


def batch_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(f, g, calls, reps):
    for _ in range(3):
        f()
        g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(batch_ms(f, calls))
        tg.append(batch_ms(g, calls))
    tf.sort()
    tg.sort()
    return dict(median=1e3 * tf[len(tf) // 2], min=1e3 * tf[0], max=1e3 * tf[-1]), \
        dict(median=1e3 * tg[len(tg) // 2], min=1e3 * tg[0], max=1e3 * tg[-1])


def kernel_times(path):
    """{jacobian: average microseconds} of k_reproject from a rocprofv3 kernel stats CSV"""
    out = {}
    for r in csv.DictReader(open(path)):
        if "k_reproject<" in r["Name"]:
            jac = "k_reproject<true" in r["Name"].replace(" ", "")
            out[jac] = dict(avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, calls=int(r["Calls"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--kernel-stats", help="kernel stats CSV of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    from wgsr import frontend
    dev = torch.device("cuda:0")
    E, frames, ht, wd = (8, 4, 12, 16) if args.small else (96, 24, 48, 64)
    g = torch.Generator(device=dev).manual_seed(3)
    from lietorch import SE3
    xi = 0.05 * torch.randn(frames, 6, device=dev, generator=g)
    with torch.no_grad():
        poses = SE3.exp(xi).data.contiguous()
    disps = (0.3 + 1.5 * torch.rand(frames, ht, wd, device=dev, generator=g)).contiguous()
    intr = torch.tensor([wd * 0.8, wd * 0.8, wd / 2 - 0.5, ht / 2 - 0.5], device=dev).repeat(frames, 1).contiguous()
    ii = (torch.arange(E, device=dev) % frames).contiguous()
    jj = ((ii + 1 + torch.arange(E, device=dev) // frames) % frames).contiguous()
    res = {"device": torch.cuda.get_device_name(0),
           "problem": dict(edges=E, frames=frames, maps=f"{ht}x{wd}", calls_per_batch=args.calls, repeats=args.reps)}
    ktimes = kernel_times(args.kernel_stats) if args.kernel_stats else {}
    with torch.no_grad():
        for jac in (False, True):
            fused = lambda: frontend.reproject(poses, disps, intr, ii, jj, jacobian=jac, check=False)  # noqa: E731
            comp = lambda: composed(poses, disps, intr, ii, jj, jac)  # noqa: E731
            a, b = fused(), comp()
            flat = lambda o: list(o[:2]) + (list(o[2]) if len(o) == 3 else [])  # noqa: E731
            agree = min(float(((x - y).abs() <= 1e-4 * y.abs() + 1e-4).float().mean())
                        for x, y in zip(flat(a), flat(b)))
            tf, tc = alternate(fused, comp, args.calls, args.reps)
            ops, group_launches = count_device_ops(comp)
            nbytes = E * ht * wd * (4 + 12 + (104 if jac else 0))
            floor_us = 1e6 * nbytes / HBM_BYTES_PER_S
            rec = dict(fused_call_us=tf, composed_call_us=tc, composed_over_fused=tc["median"] / tf["median"],
                       agree=agree, fused_device_ops=1, composed_device_ops=ops,
                       composed_group_kernel_launches=group_launches, unique_bytes=nbytes,
                       byte_model_floor_us=floor_us)
            if jac in ktimes:
                rec["kernel_us"] = ktimes[jac]
                rec["fraction_of_byte_model"] = floor_us / ktimes[jac]["avg_us"]
            else:
                rec["kernel_us"] = rec["fraction_of_byte_model"] = "not measured"
            res["jacobian" if jac else "plain"] = rec
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
