#!/usr/bin/env python
"""droid_backends.ba on the MI355X path (csrc/droid_ba.hip) against a torch
composition of the same algorithm on the same GPU.

Two graphs at the tracker's 48 x 64 (1/8) resolution, ``iterations=2``, full
and ``motion_only``:

* frontend-like   12 free frames (one fixed before them), band graph of
                  radius 3: about 80 edges
* backend-like    120 free frames, band graph of radius 6: about 1400 edges

The torch composition: batched tensor ops for the linearisation, ``einsum`` /
``index_add_`` assembly, a dense per-frame coupling tensor and ``bmm`` for the
Schur complement, ``torch.linalg.cholesky_ex`` in fp64 (its graph structures --
kx, the slot map -- are built outside the timed region).

Device time per call from HIP events (median of repeats after warm-up); the
HIP op's per-stage times (linearise, Schur/assembly, solve, back-substitute)
from events the library records around its stages, for one iteration (a call
with ``iterations=1``).  Prints one JSON object; ``--out FILE`` also writes it there;
``--small`` shrinks both graphs (a quick check of the tool itself).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "wildgs-slam-blackwell_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_droid import make_frames, quat_rotate, relative, timed  # noqa: E402

MIN_DEPTH, ALPHA = 0.25, 0.05


def quat_mul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def conj(q):
    return q * q.new_tensor([-1, -1, -1, 1])


def rays(ht, wd, intr):
    v, u = torch.meshgrid(torch.arange(ht, dtype=torch.float32, device=intr.device),
                          torch.arange(wd, dtype=torch.float32, device=intr.device), indexing="ij")
    return torch.stack([(u - intr[2]) / intr[0], (v - intr[3]) / intr[1], torch.ones_like(u)], -1).reshape(-1, 3)


def project(poses, disps, intr, ii, jj):
    """proj [N, 2, HW] of every edge's source pixels in its target frame."""
    q, t = relative(poses, ii, jj)
    h = disps[ii].reshape(len(ii), -1)
    Y = quat_rotate(q, rays(disps.shape[1], disps.shape[2], intr)[None].expand(len(ii), -1, -1)) \
        + h[..., None] * t[:, None, :]
    d = torch.where(Y[..., 2] >= MIN_DEPTH, 1 / Y[..., 2], torch.zeros_like(h))
    return torch.stack([intr[0] * d * Y[..., 0] + intr[2], intr[1] * d * Y[..., 1] + intr[3]], 1)


def retract(poses, dx):
    tau, phi = dx[:, :3], dx[:, 3:]
    th2 = (phi * phi).sum(-1, keepdim=True)
    th = th2.sqrt()
    small, ths, th2s = th2 < 1e-8, th.clamp(min=1e-12), th2.clamp(min=1e-24)
    imag = torch.where(small, 0.5 - th2 / 48 + th2 * th2 / 3840, torch.sin(0.5 * th) / ths)
    real = torch.where(small, 1 - th2 / 8 + th2 * th2 / 384, torch.cos(0.5 * th))
    dq = torch.cat([imag * phi, real], -1)
    c1 = torch.cross(phi, tau, dim=-1)
    c2 = torch.cross(phi, c1, dim=-1)
    big = th > 1e-4
    dt = tau + torch.where(big, (1 - torch.cos(th)) / th2s, 0 * th) * c1 \
        + torch.where(big, (th - torch.sin(th)) / (ths * th2s), 0 * th) * c2
    t1 = quat_rotate(dq, poses[:, None, :3])[:, 0] + dt
    return torch.cat([t1, quat_mul(dq, poses[:, 3:])], -1)


class TorchBA:
    """The algorithm of csrc/droid_ba.hip as a torch composition."""

    def __init__(self, disps, ii, jj, t0, t1):
        dev = disps.device
        self.t0, self.t1, self.P = t0, t1, t1 - t0
        self.kx = torch.unique(torch.cat([torch.arange(t0, t1, device=dev), ii]))
        self.K = len(self.kx)
        slot = torch.full((disps.shape[0],), -1, dtype=torch.int64, device=dev)
        slot[self.kx] = torch.arange(self.K, device=dev)
        P = self.P
        free = lambda f: torch.where((f >= t0) & (f < t1), f - t0, torch.full_like(f, P))  # noqa: E731  (P: dropped)
        self.pi, self.pj, self.ki = free(ii), free(jj), slot[ii]

    def step(self, poses, disps, intr, sens, targets, weights, eta, ii, jj, lm, ep, motion_only):
        N, (ht, wd), P, K = len(ii), disps.shape[1:], self.P, self.K
        HW = ht * wd
        fx, fy, cx, cy = intr.unbind()
        q, t = relative(poses, ii, jj)
        h = disps[ii].reshape(N, HW)
        Y = quat_rotate(q, rays(ht, wd, intr)[None].expand(N, -1, -1)) + h[..., None] * t[:, None, :]
        x, y, z = Y.unbind(-1)
        ok = z >= MIN_DEPTH
        zero = torch.zeros_like(z)
        d = torch.where(ok, 1 / z, zero)
        d2 = d * d
        w2 = torch.where(ok[:, None], 0.001 * weights.reshape(N, 2, HW), zero[:, None])
        r = targets.reshape(N, 2, HW) - torch.stack([fx * d * x + cx, fy * d * y + cy], 1)
        Jj = torch.stack([
            torch.stack([fx * h * d, zero, -fx * x * h * d2, -fx * x * y * d2, fx * (1 + x * x * d2), -fx * y * d], 1),
            torch.stack([zero, fy * h * d, -fy * y * h * d2, -fy * (1 + y * y * d2), fy * x * y * d2, fy * x * d], 1)],
            1)                                                                   # [N, 2, 6, HW]
        Jz = torch.stack([fx * (t[:, 0:1] * d - t[:, 2:3] * x * d2), fy * (t[:, 1:2] * d - t[:, 2:3] * y * d2)], 1)
        a, b = Jj[:, :, :3].permute(0, 1, 3, 2), Jj[:, :, 3:].permute(0, 1, 3, 2)     # [N, 2, HW, 3]
        qi = conj(q)
        tt = t[:, None, None, :].expand_as(a)
        Ji = -torch.cat([quat_rotate(qi, a.reshape(N, 2 * HW, 3)).reshape(N, 2, HW, 3),
                         quat_rotate(qi, (b + torch.cross(a, tt, dim=-1)).reshape(N, 2 * HW, 3)).reshape(N, 2, HW, 3)],
                        -1).permute(0, 1, 3, 2)
        J = torch.cat([Ji, Jj], 2)                                               # [N, 2, 12, HW]
        wJ = w2[:, :, None] * J
        H = torch.einsum("nrap,nrbp->nab", wJ, J)
        v = torch.einsum("nrap,nrp->na", wJ, r)
        # the pose block (index P collects the fixed poses' rows and columns)
        A = torch.zeros((P + 1) * (P + 1), 6, 6, dtype=torch.float64, device=poses.device)
        av = torch.zeros(P + 1, 6, dtype=torch.float64, device=poses.device)
        ends = (self.pi, self.pj)
        for xi, px in enumerate(ends):
            av.index_add_(0, px, v[:, 6 * xi:6 * xi + 6].double())
            for yi, py in enumerate(ends):
                A.index_add_(0, px * (P + 1) + py, H[:, 6 * xi:6 * xi + 6, 6 * yi:6 * yi + 6].double())
        Hr = A.view(P + 1, P + 1, 6, 6)[:P, :P].permute(0, 2, 1, 3).reshape(6 * P, 6 * P)
        g = av[:P].reshape(6 * P)
        if not motion_only:
            E = (wJ * Jz[:, :, None]).sum(1)                                     # [N, 12, HW]
            Ce, be = (w2 * Jz * Jz).sum(1), (w2 * r * Jz).sum(1)
            m = sens[self.kx].reshape(K, HW) > 0
            C = torch.zeros(K, HW, device=poses.device).index_add_(0, self.ki, Ce) \
                + torch.where(m, torch.full_like(eta.reshape(K, HW), ALPHA), eta.reshape(K, HW))
            w = torch.zeros(K, HW, device=poses.device).index_add_(0, self.ki, be) \
                - torch.where(m, ALPHA * (disps[self.kx] - sens[self.kx]).reshape(K, HW), torch.zeros_like(C))
            Q = 1 / C
            M = torch.zeros(K * (P + 1), 6, HW, device=poses.device)
            M.index_add_(0, self.ki * (P + 1) + self.pi, E[:, :6])
            M.index_add_(0, self.ki * (P + 1) + self.pj, E[:, 6:])
            Mv = M.view(K, P + 1, 6, HW)[:, :P].reshape(K, 6 * P, HW)
            S = torch.bmm(Mv * Q[:, None, :], Mv.transpose(1, 2)).double().sum(0)
            s = (Mv * (Q * w)[:, None, :]).sum(2).double().sum(0)
            Hr, g = Hr - S, g - s
        idx = torch.arange(6 * P, device=poses.device)
        Hr = Hr.clone()
        Hr[idx, idx] = Hr[idx, idx] + (ep + lm * Hr[idx, idx])
        L, info = torch.linalg.cholesky_ex(Hr)
        dx = torch.cholesky_solve(g[:, None], L)[:, 0]
        dx = torch.where(info == 0, dx, torch.zeros_like(dx)).float().reshape(P, 6)
        dz = None
        if not motion_only:
            # (pose t0's own step does not enter dz: the op's recorded quirk)
            dz = Q * (w - torch.einsum("kcp,c->kp", Mv[:, 6:], dx.reshape(-1)[6:]))
            disps[self.kx] += dz.reshape(K, ht, wd)
        poses[self.t0:self.t1] = retract(poses[self.t0:self.t1], dx)
        return dx, dz

    def run(self, poses, disps, intr, sens, targets, weights, eta, ii, jj, iterations, lm, ep, motion_only):
        for _ in range(iterations):
            out = self.step(poses, disps, intr, sens, targets, weights, eta, ii, jj, lm, ep, motion_only)
        return out


def make_problem(P, radius, ht, wd, dev, seed=0):
    num = P + 1
    poses, disps, intr = make_frames(num, ht, wd, dev, seed)
    i, j = torch.meshgrid(torch.arange(num), torch.arange(num), indexing="ij")
    keep = (i != j) & ((i - j).abs() <= radius)
    ii, jj = i[keep].to(dev).contiguous(), j[keep].to(dev).contiguous()
    g = torch.Generator().manual_seed(seed + 1)
    true = retract(poses, (4e-3 * (2 * torch.rand(num, 6, generator=g) - 1)).to(dev))
    N = len(ii)
    targets = (project(true, disps, intr, ii, jj).reshape(N, 2, ht, wd)
               + 0.05 * torch.randn(N, 2, ht, wd, generator=g).to(dev)).contiguous()
    weights = (0.05 + 0.95 * torch.rand(N, 2, ht, wd, generator=g)).to(dev).contiguous()
    K = num if radius >= 1 else P
    eta = (0.2 * torch.rand(K, ht, wd, generator=g) + 1e-7).to(dev).contiguous()
    return dict(poses=poses, disps=disps, intr=intr, sens=torch.zeros_like(disps), targets=targets, weights=weights,
                eta=eta, ii=ii, jj=jj, t0=1, t1=num)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # the tool still reports its times
        return [f"unavailable: {e}"]


def bench_graph(name, p, reps):
    import droid_backends
    from wgsr import _lib
    L = _lib.load()
    out = {"free_frames": p["t1"] - p["t0"], "edges": len(p["ii"]), "frame": f"{p['disps'].shape[1]}x{p['disps'].shape[2]}"}
    ref = TorchBA(p["disps"], p["ii"], p["jj"], p["t0"], p["t1"])
    assert ref.K == p["eta"].shape[0]
    for mode, motion_only in (("full", False), ("motion_only", True)):
        state = lambda: (p["poses"].clone(), p["disps"].clone())  # noqa: E731

        def hip(ps=None, ds=None, **kw):
            ps, ds = (ps, ds) if ps is not None else state()
            return droid_backends.ba(ps, ds, p["intr"], p["sens"], p["targets"], p["weights"], p["eta"], p["ii"],
                                     p["jj"], p["t0"], p["t1"], 2, 1e-4, 0.1, motion_only, False, **kw)

        def tor(ps=None, ds=None):
            ps, ds = (ps, ds) if ps is not None else state()
            return ref.run(ps, ds, p["intr"], p["sens"], p["targets"], p["weights"], p["eta"], p["ii"], p["jj"], 2,
                           1e-4, 0.1, motion_only)

        # agreement of the two on the final state
        ph, dh = state()
        hip(ph, dh)
        pt, dt = state()
        tor(pt, dt)
        agree = {"poses_max_abs_diff": float((ph - pt).abs().max()), "disps_max_abs_diff": float((dh - dt).abs().max()),
                 "pose_step_max": float((ph - p["poses"]).abs().max())}
        hip_ms = timed(lambda: hip(check=False), reps)
        torch_ms = timed(tor, max(3, reps // 3))
        # per-stage device times of the last timed calls: events recorded by the library
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        for e in evs:
            e.record()
        torch.cuda.synchronize()
        handles = (ctypes.c_void_p * 5)(*[e.cuda_event for e in evs])
        stages = {"linearise": [], "schur_assembly": [], "solve": [], "back_substitute_retract": []}
        for _ in range(reps):
            # one iteration per call, so that each event is recorded once
            ps, ds = state()
            L.wgsr_droid_ba_stage_events(handles)
            droid_backends.ba(ps, ds, p["intr"], p["sens"], p["targets"], p["weights"], p["eta"], p["ii"], p["jj"],
                              p["t0"], p["t1"], 1, 1e-4, 0.1, motion_only, False, check=False)
            L.wgsr_droid_ba_stage_events(None)
            torch.cuda.synchronize()
            for k, key in enumerate(stages):
                stages[key].append(evs[k].elapsed_time(evs[k + 1]))
        med = {k: sorted(v)[len(v) // 2] for k, v in stages.items()}
        total = sum(med.values())
        out[mode] = {"hip_ms": hip_ms, "torch_ms": torch_ms, "torch_over_hip": torch_ms / hip_ms, "agree": agree,
                     "stage_ms_one_iteration": med, "solve_share_of_iteration": med["solve"] / total}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ht, wd = (12, 16) if a.small else (48, 64)
    res = {"device": torch.cuda.get_device_name(0), "clocks": clocks(), "iterations": 2,
           "timing": "HIP events, median after 2 warm-up calls; hip_ms includes the workspace allocation and the "
                     "two state copies each call starts from, torch_ms the same copies"}
    res["frontend_like"] = bench_graph("frontend", make_problem(4 if a.small else 12, 3, ht, wd, dev), a.reps)
    res["backend_like"] = bench_graph("backend", make_problem(20 if a.small else 120, 6, ht, wd, dev), a.reps)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
