"""Element-wise reference for the mapper-side kernels that had none:
csrc/tracking.hip (k_track_loss, k_grad_intensity, k_grad_block,
k_pose_step), csrc/dino.hip and csrc/mapping.hip.  The cases (seeded, cached
per case; treat every field as read-only), the float64 oracle and fp32
restatement runs, and the checks.

The bound and its machinery are tests/_loss_elementwise_ref.py's:

    |got - oracle64| <= MARGIN * spread + 1e-6 * scale,
    spread = max |restatement32 - oracle64|,  scale = max |oracle64|,

element-wise with the tensor's maxima and stratified by float64 magnitude
(check_tensor).  Every oracle here is a plain numpy / torch-CPU restatement of
the formulas in the kernel's header comment, written once, dtype-generic, and
run in float64 and in float32.

Decisions.  A pixel or row whose float64 oracle puts a decision within DELTA
of its threshold is excluded from the comparison (it must still be finite).
DELTA is MARGIN x the largest |fp32 - float64| deviation of the compared
quantity on that case (printed with the case's counts), never a free number.
A difference that is exactly zero in float64 AND in float32 is structural
(an element compared with itself, two masked zeros, three bit-equal scales)
and is no decision.  tests/test_map_elementwise_ref.py asserts the caps:
tracking loss and mapping loss 1 % of the pixels, gradient mask 2 %,
activation backward 1 % of the rows, DINO zero rows.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from _loss_elementwise_ref import GROUPS, MARGIN, MIN_GROUP, Report, check_tensor, strata  # noqa: F401

# per-tensor margins above MARGIN ("<family>:<tensor>"), each with its cause
# and the ratio err / spread measured against the float64 oracle
MARGINS: dict = {}
CAP_LOSS = 0.01      # tracking loss, mapping loss (pixels), activation backward (rows)
CAP_MASK = 0.02      # gradient mask (the depth-filter tests' cap)
F32 = lambda v: float(np.float32(v))  # noqa: E731  (a float argument as the kernel receives it)
RGB_TH = F32(0.01)
WGROUP = 256         # kTBlock, kMapBlock: pixels / Gaussians per workgroup


# ---- guarded device buffers of the GPU tests (tests/test_gpu_encoders.py's FILL / GUARD)
GUARD = 64
FILL = -1.2345e30


class Guarded:
    """A device buffer of ``shape`` filled with FILL, with GUARD more elements behind it."""

    def __init__(self, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape))
        self.fill = FILL if dtype.is_floating_point else -12345
        self.whole = torch.full((n + GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.whole[:n].view(shape)
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).view(shape))

    def ptr(self):
        return self.t.data_ptr()

    def read(self, written=True):
        """-> numpy; asserts the guard untouched and (``written``) every element written."""
        assert bool((self.whole[self.t.numel():] == self.fill).all()), "guard elements were written"
        out = self.t.cpu().numpy()
        if written:
            assert not (out == np.asarray(self.fill, out.dtype)).any(), "output elements were left unwritten"
        return out


def _check(rep, family, name, got, o64, o32, keep=None, margin=None):
    m = margin if margin is not None else MARGINS.get(f"{family}:{name}", MARGIN)
    check_tensor(rep, name, got, o64, o32, keep=keep, margin=m, family=family)


def _np64(t):
    return None if t is None else t.detach().numpy().astype(np.float64)


def _dev(a, b):
    """max |fp32 - float64| of a compared quantity."""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) if np.size(a) else 0.0


def _near0(d64, d32, delta):
    """|d64| within delta of 0, unless the difference is exactly 0 in both precisions."""
    return (np.abs(d64) <= delta) & ~((d64 == 0) & (d32 == 0))


def wg_sums(x, dtype=np.float64):
    """Per-workgroup sums of a per-pixel / per-row quantity."""
    x = np.asarray(x, dtype).reshape(-1)
    nb = (x.size + WGROUP - 1) // WGROUP
    return np.array([x[b * WGROUP:(b + 1) * WGROUP].sum(dtype=dtype) for b in range(nb)], np.float64)


# ------------------------------------------------------------ tracking loss

TRACK_SHAPES = ((1, 1), (7, 37), (16, 16), (33, 129))
TRACK_MODES = ("gm+unc", "none", "gm", "unc")
TRACK_TENSORS = ("d_image", "d_opacity")
TRACK_SCALARS = ("loss", "d_exposure_a", "d_exposure_b")
_TRACK_SEED = {(1, 1): 1, (7, 37): 2, (16, 16): 3, (33, 129): 4}


def track_case_names():
    return [f"{h}x{w}-{m}" for h, w in TRACK_SHAPES for m in TRACK_MODES]


def track_frame(H, W, seed):
    """gt with a band under the rgb threshold, an uncertainty with a band above
    sqrt(5) (weight 0.5 / u^2 under 0.1), a 0 / 1 gradient mask, non-zero
    exposures."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    gt[:, :, : max(W // 5, 0)] = 0.002
    ren = (gt + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    opa = torch.rand(1, H, W, generator=g)
    gm = (torch.rand(1, H, W, generator=g) > 0.3).float()
    unc = torch.rand(H, W, generator=g) * 1.7 + 0.3
    hi = 2.4 + 0.5 * torch.rand(H, W, generator=g)
    unc[H // 2:, W // 2: W - W // 8] = hi[H // 2:, W // 2: W - W // 8]   # (the last pixels keep their weight)
    if H * W == 1:
        unc[:] = 0.8
    return dict(gt=gt, ren=ren, opa=opa, gm=gm, unc=unc, ea=torch.tensor([0.07]), eb=torch.tensor([-0.03]))


def track_forward(v, use_gm, use_unc):
    """get_loss_tracking_rgb (k_track_loss's header) -> (loss, residual, gt sum, weight)."""
    dt = v["ren"].dtype
    image_ab = torch.exp(v["ea"]) * v["ren"] + v["eb"]
    gsum = (v["gt"][0] + v["gt"][1]) + v["gt"][2]
    m = (gsum > RGB_TH).to(dt)[None]
    if use_gm:
        m = m * v["gm"]
    r = image_ab * m - v["gt"] * m
    l1 = v["opa"] * torch.abs(r)
    w = None
    if use_unc:
        w = (1.0 / (v["unc"][None] * v["unc"][None])) * 0.5
        w = torch.where(w < F32(0.1), torch.zeros_like(w), w)
        l1 = l1 * w
    return l1.mean(), r, gsum, w, m, l1


def track_run(t, use_gm, use_unc, dtype, drop_last_group=False):
    v = {k: x.to(dtype) for k, x in t.items()}
    for k in ("ren", "opa", "ea", "eb"):
        v[k] = v[k].clone().requires_grad_(True)
    loss, r, gsum, w, m, l1 = track_forward(v, use_gm, use_unc)
    loss.backward()
    if drop_last_group:  # the tooth: the last partial workgroup's pixels left out of the loss sum
        flat = l1.detach().reshape(3, -1)
        n = flat.shape[1]
        loss = flat[:, : (n // WGROUP) * WGROUP].sum() / (3 * n)
    wraw = None if not use_unc else _np64((1.0 / (v["unc"] * v["unc"])) * 0.5)
    return dict(loss=_np64(loss), d_image=_np64(v["ren"].grad), d_opacity=_np64(v["opa"].grad),
                d_exposure_a=_np64(v["ea"].grad), d_exposure_b=_np64(v["eb"].grad), r=_np64(r), gsum=_np64(gsum),
                w=wraw, m=_np64(m)[0])


@functools.lru_cache(maxsize=None)
def track_case(name):
    shape_s, mode = name.split("-")
    H, W = (int(x) for x in shape_s.split("x"))
    use_gm, use_unc = mode in ("gm+unc", "gm"), mode in ("gm+unc", "unc")
    t = track_frame(H, W, _TRACK_SEED[(H, W)])
    o64, o32 = track_run(t, use_gm, use_unc, torch.float64), track_run(t, use_gm, use_unc, torch.float32)
    delta = dict(residual=MARGIN * _dev(o32["r"], o64["r"]), gt_sum=MARGIN * _dev(o32["gsum"], o64["gsum"]))
    near = (_near0(o64["r"], o32["r"], delta["residual"]) & (o64["m"] != 0)[None]).any(0)
    near |= np.abs(o64["gsum"] - RGB_TH) <= delta["gt_sum"]
    census = dict(rgb_mask=o64["gsum"] > RGB_TH)
    if use_gm:
        census["grad_mask"] = t["gm"].numpy()[0] > 0
    if use_unc:
        delta["weight"] = MARGIN * _dev(o32["w"], o64["w"])
        near |= np.abs(o64["w"] - F32(0.1)) <= delta["weight"]
        census["weight_cut"] = o64["w"] < F32(0.1)
    return SimpleNamespace(name=name, H=H, W=W, use_gm=use_gm, use_unc=use_unc, t=t, o64=o64, o32=o32, near=near,
                           delta=delta, census=census)


def track_check(c, got, margin=None):
    """``got``: dict of TRACK_TENSORS ([3, H, W], [1, H, W]) and TRACK_SCALARS."""
    rep = Report("track " + c.name)
    print(f"  DELTA {c.delta}; {int(c.near.sum())} of {c.near.size} pixels excluded")
    for k in TRACK_TENSORS:
        keep = np.broadcast_to(~c.near, c.o64[k].shape)
        _check(rep, "track", k, got[k], c.o64[k], c.o32[k], keep=keep, margin=margin)
    for k in TRACK_SCALARS:
        if k == "loss" or not c.near.any():  # (a sign flip of an excluded pixel moves the exposure sums)
            _check(rep, "track", k, got[k], c.o64[k], c.o32[k], margin=margin)
    return rep.finish()


# ------------------------------------------------------------ gradient mask

EPS_GREY = F32(0.01)
# name -> (H, W, image kind, edge_threshold, what)
GMASK_CASES = {
    "2x2": (2, 2, "dark", 4, "no blocks, all border"),
    "31x70": (31, 70, "dark", 4, "no blocks (bh = 0)"),
    "70x31": (70, 31, "dark", 4, "no blocks (bw = 0)"),
    "40x45": (40, 45, "dark", 4, "blocks of 1, remainder strips"),
    "33x65": (33, 65, "dark", 4, "blocks of 2 (1 x 2)"),
    "67x100": (67, 100, "dark", 4, "blocks of 6 (2 x 3), remainder strips"),
    "64x96": (64, 96, "dark", 4, "blocks of 6: the lower median"),
    "64x96-t1": (64, 96, "dark", 1, "blocks of 6 at edge_threshold 1"),
    "96x160": (96, 160, "dark", 4, "blocks of 15 (odd)"),
    "544x544": (544, 544, "dark", 4, "blocks of 289: more elements than threads, np = 512"),
    "64x64-flat": (64, 64, "flat", 4, "blocks of 4, whole blocks masked to 0 (median 0)"),
    "64x66-columns": (64, 66, "columns", 4, "blocks of 4 with 4 x median >= 1: all zero"),
    # (an image within [0, 1] has intensities under 0.71, so with 1 <= t nothing is above t and the second
    # assignment has nothing to undo; isolated pixels of 20 put intensities of ~6 over a t of 1.96)
    "64x66-spikes": (64, 66, "spikes", 4, "blocks of 4 with 1 <= t < v: set to 1, then to 0"),
}


def gmask_image(H, W, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "columns":  # grey columns 1, 1, 0.02, 0.02, ...: the intensity is 0.49 off the first column
        col = torch.tensor([1.0, 1.0, 0.02, 0.02]).repeat((W + 3) // 4)[:W]
        return col.view(1, 1, W).expand(3, H, W).contiguous().numpy()
    if kind == "spikes":
        img = torch.from_numpy(gmask_image(H, W, "columns", seed)).clone()
        img[:, 3::8, 5::8] = 20.0
        return img.numpy()
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = 0.5 + 0.3 * torch.sin(9 * xx) * torch.cos(7 * yy)
    img = (torch.stack([base, base * 0.8, base * 0.6]) + 0.15 * torch.rand(3, H, W, generator=g)).clamp(0.06, 1)
    dark = 0.004 * torch.rand(3, H, W, generator=g)
    if kind == "flat":  # a dark patch over whole blocks and parts of blocks
        sl = [(slice(7, 41), slice(9, 51))]
    else:  # a dark patch and a dark border (two sides: the reflect-padded edge sees both values)
        b = max(1, min(H, W) // 16)
        sl = [(slice(H // 3, H // 2 + 1), slice(W // 4, W // 2 + 1)), (slice(H - b, H), slice(None)),
              (slice(None), slice(W - b, W))]
        if min(H, W) <= 2:
            sl = [(slice(0, 1), slice(0, 1))]
    for s in sl:
        img[(slice(None), *s)] = dark[(slice(None), *s)]
    return img.contiguous().numpy()


def _pad1(a, mode):
    return np.pad(a, 1, mode=mode)


def gmask_intensity(img, dtype, top="reflect"):
    """k_grad_intensity's header: Scharr magnitude of the grey image where the
    whole reflect-padded 3 x 3 neighbourhood is above eps -> (intensity, grey).
    ``top``: the tooth's padding of the top row."""
    x = img.astype(dtype)
    grey = ((x[0] + x[1]) + x[2]) * dtype(1.0 / 3.0) if dtype is np.float32 else ((x[0] + x[1]) + x[2]) / 3.0
    p = _pad1(grey, "reflect")
    if top != "reflect":
        p[0] = _pad1(grey, "edge")[0]
    H, W = grey.shape
    v = [[p[dy:dy + H, dx:dx + W] for dx in range(3)] for dy in range(3)]
    ok = np.ones((H, W), bool)
    for row in v:
        for e in row:
            ok &= np.abs(e) > EPS_GREY
    c3, c10, n = dtype(3), dtype(10), dtype(0.03125)
    cx = c3 * v[0][0] + c10 * v[0][1] + c3 * v[0][2] - c3 * v[2][0] - c10 * v[2][1] - c3 * v[2][2]
    cy = c3 * v[0][0] - c3 * v[0][2] + c10 * v[1][0] - c10 * v[1][2] + c3 * v[2][0] - c3 * v[2][2]
    m = ok.astype(dtype)
    gv, gh = (n * cx) * m, (n * cy) * m
    return np.sqrt(gv * gv + gh * gh), grey


def gmask_blocks(inten, mult, dtype, median="lower", keep_one=False):
    """k_grad_block's header: per block of the 32 x 32 grid, t = multiplier x
    the lower median; block[v > t] = 1, then block[v <= t] = 0 (so a block with
    1 <= t ends all zero) -> (mask, v - t per pixel, t per pixel).  ``median``
    and ``keep_one``: the teeth."""
    H, W = inten.shape
    bh, bw = H // 32, W // 32
    out = inten.astype(dtype).copy()
    d = np.full((H, W), np.nan)
    tt = np.full((H, W), np.nan)
    if bh == 0 or bw == 0:
        return out, d, tt
    for r in range(32):
        for c in range(32):
            sl = (slice(r * bh, (r + 1) * bh), slice(c * bw, (c + 1) * bw))
            v = out[sl]
            s = np.sort(v.reshape(-1))
            n = s.size
            med = s[(n - 1) // 2] if median == "lower" else s[n // 2]
            t = med * dtype(mult)
            hi = dtype(1) if (keep_one or not (dtype(1) <= t)) else dtype(0)
            d[sl] = v.astype(np.float64) - np.float64(t)
            tt[sl] = t
            out[sl] = np.where(v > t, hi, dtype(0))
    return out, d, tt


def gmask_run(img, mult, dtype, **teeth):
    inten, grey = gmask_intensity(img, dtype, top=teeth.get("top", "reflect"))
    mask, d, t = gmask_blocks(inten, mult, dtype, median=teeth.get("median", "lower"),
                              keep_one=teeth.get("keep_one", False))
    return dict(mask=mask.astype(np.float64), inten=inten.astype(np.float64), grey=grey.astype(np.float64), d=d, t=t)


def _dilate3_reflect(b):
    p = _pad1(b, "reflect") if min(b.shape) > 1 else _pad1(b, "edge")
    H, W = b.shape
    out = np.zeros_like(b)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + H, dx:dx + W]
    return out


@functools.lru_cache(maxsize=None)
def gmask_case(name):
    H, W, kind, mult, what = GMASK_CASES[name]
    img = gmask_image(H, W, kind, 100 + H + W)
    o64, o32 = gmask_run(img, mult, np.float64), gmask_run(img, mult, np.float32)
    bh, bw = H // 32, W // 32
    inside = np.zeros((H, W), bool)
    if bh and bw:
        inside[:32 * bh, :32 * bw] = True
    delta = dict(grey=MARGIN * _dev(o32["grey"], o64["grey"]))
    eps_near = _dilate3_reflect(np.abs(np.abs(o64["grey"]) - EPS_GREY) <= delta["grey"])
    delta["intensity"] = MARGIN * _dev(o32["inten"][~eps_near], o64["inten"][~eps_near])
    flagged = eps_near.copy()
    if inside.any():
        ok = inside & ~eps_near
        delta["v_minus_t"] = MARGIN * _dev(o32["d"][ok], o64["d"][ok])
        flagged |= inside & _near0(np.nan_to_num(o64["d"]), np.nan_to_num(o32["d"]), delta["v_minus_t"])
        # a block whose median may be another element altogether (an eps decision
        # inside it), or whose t sits at 1, is flagged whole
        for r in range(32):
            for c in range(32):
                sl = (slice(r * bh, (r + 1) * bh), slice(c * bw, (c + 1) * bw))
                t64, t32 = o64["t"][sl].flat[0], o32["t"][sl].flat[0]
                if eps_near[sl].any() or abs(t64 - 1.0) <= MARGIN * abs(t32 - t64) + delta["v_minus_t"]:
                    flagged[sl] = True
    return SimpleNamespace(name=name, H=H, W=W, mult=mult, img=img, o64=o64, o32=o32, inside=inside,
                           eps_near=eps_near, flagged=flagged, delta=delta, what=what)


def gmask_check(c, got, margin=None):
    """``got``: the [H, W] output of wgsr_grad_mask.  Off the flagged pixels the
    block pixels agree exactly with the float64 oracle and the raw-intensity
    pixels are inside the bound."""
    rep = Report("grad_mask " + c.name)
    got = np.asarray(got, np.float64).reshape(c.H, c.W)
    print(f"  DELTA {c.delta}; {int(c.flagged.sum())} of {c.flagged.size} pixels flagged")
    if not np.all(np.isfinite(got)):
        rep.fails.append("mask: not finite")
        return rep.finish()
    blk = c.inside & ~c.flagged
    bad = blk & (got != c.o64["mask"])
    print(f"  RATIO grad_mask {c.name} block pixels: {int(bad.sum())} unflagged mismatches of {int(blk.sum())}")
    if bad.any():
        y, x = np.argwhere(bad)[0]
        rep.fails.append(f"mask: {int(bad.sum())} unflagged block pixels differ, first ({y}, {x}): "
                         f"{got[y, x]} against {c.o64['mask'][y, x]}")
    if (c.inside & ~np.isin(got, (0.0, 1.0))).any():
        rep.fails.append("mask: a block pixel is neither 0 nor 1")
    raw = ~c.inside
    if raw.any():
        _check(rep, "grad_mask", "intensity", got[raw], c.o64["inten"][raw], c.o32["inten"][raw],
               keep=~c.eps_near[raw], margin=margin)
    return rep.finish()


# ---------------------------------------------------------------- pose step

POSE_GROUPS = {"R": slice(0, 9), "T": slice(9, 12), "exposures": slice(12, 14), "exp_avg": slice(16, 24),
               "exp_avg_sq": slice(24, 32), "viewmatrix": slice(32, 48), "projmatrix": slice(48, 64),
               "campos": slice(64, 67), "tau": slice(67, 68)}
POSE_ANGLES = (0.0, 5e-6, 2e-5, 1e-2, 1.0)   # 0 and 5e-6: the series branch; 2e-5: just above it (1 - cos cancels)
POSE_STEPS = (1, 7)
POSE_NPART = (1, 3, 1500)
POSE_CONV_TH = F32(1e-4)
POSE_BETAS = (F32(0.9), F32(0.999))
POSE_EPS = F32(1e-8)


def pose_case_names():
    return [f"a{a:g}_s{s}_n{n}" for a in POSE_ANGLES for s in POSE_STEPS for n in POSE_NPART]


def pose_step(st, dtau, part, proj, lr, step, dtype, camera_only=False, tooth=None):
    """k_pose_step's header and body in ``dtype`` -> (state [68] as float64, converged,
    the update's angle), or with ``camera_only`` (state, None).  ``st``'s pad floats 14, 15
    are carried through."""
    f = dtype
    st = np.asarray(st, f).copy()
    proj = np.asarray(proj, f).reshape(4, 4)
    R, T = st[0:9].reshape(3, 3).copy(), st[9:12].copy()

    def camera(R, T):
        Wv = np.zeros((4, 4), f)
        Wv[:3, :3] = R.T
        Wv[3, :3] = T
        Wv[3, 3] = 1
        st[32:48] = Wv.reshape(-1)
        st[48:64] = (Wv @ proj).reshape(-1)
        cc = T @ R
        st[64:67] = cc if tooth == "campos_sign" else -cc
    if camera_only:
        camera(R, T)
        return st.astype(np.float64), None
    b1, b2 = f(POSE_BETAS[0]), f(POSE_BETAS[1])
    bc1 = f(1.0 - float(POSE_BETAS[0]) ** step)
    bc2s = f(np.sqrt(1.0 - float(POSE_BETAS[1]) ** step))
    if tooth == "no_bc2":
        bc2s = f(1)
    part = np.asarray(part, f).reshape(-1, 3)
    ga, gb = part[:, 1].sum(dtype=f), part[:, 2].sum(dtype=f)
    d = np.asarray(dtau, f)
    g = np.array([d[3], d[4], d[5], d[0], d[1], d[2], ga, gb], f)
    lrs = np.array([lr[0]] * 3 + [lr[1]] * 3 + [lr[2]] * 2, f)
    m = b1 * st[16:24] + (f(1) - b1) * g
    v = b2 * st[24:32] + (f(1) - b2) * g * g
    st[16:24], st[24:32] = m, v
    denom = np.sqrt(v) / bc2s + f(POSE_EPS)
    p0 = np.array([0, 0, 0, 0, 0, 0, st[12], st[13]], f)
    pnew = p0 - (lrs / bc1) * (m / denom)
    st[12], st[13] = pnew[6], pnew[7]
    th, rho = pnew[0:3], pnew[3:6]
    Wm = np.array([[0, -th[2], th[1]], [th[2], 0, -th[0]], [-th[1], th[0], 0]], f)
    W2 = Wm @ Wm
    angle = np.sqrt(th[0] * th[0] + th[1] * th[1] + th[2] * th[2])
    I = np.eye(3, dtype=f)
    if angle < f(F32(1e-5)):
        Rx = I + Wm + f(0.5) * W2
        Vm = I + f(0.5) * Wm + f(1.0 / 6.0) * W2
    else:
        sa, ca, a2 = np.sin(angle), np.cos(angle), angle * angle
        c1, c2, c3 = sa / angle, (f(1) - ca) / a2, (angle - sa) / (a2 * angle)
        if tooth == "swap_c2c3":
            Rx, Vm = I + c1 * Wm + c2 * W2, I + Wm * c3 + W2 * c2
        else:
            Rx, Vm = I + c1 * Wm + c2 * W2, I + Wm * c2 + W2 * c3
    Rn = Rx @ R
    Tn = Rx @ T + Vm @ rho
    st[0:9], st[9:12] = Rn.reshape(-1), Tn
    tn = np.sqrt((rho * rho).sum(dtype=f) + (th * th).sum(dtype=f))
    st[67] = tn
    camera(Rn, Tn)
    return st.astype(np.float64), int(tn < f(POSE_CONV_TH)), float(angle)


def _pose_inputs(step, n_part, seed):
    """A generic state: a rotation well away from I, non-zero exposures and
    moments; dtau, the loss partials, a projection."""
    g = np.random.default_rng(seed)
    q = g.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    st = np.zeros(68, np.float32)
    st[0:9] = R.reshape(-1)
    st[9:12] = g.normal(size=3) * 1.5
    st[12:14] = (0.06, -0.04)
    st[16:24] = g.normal(size=8) * 0.05   # (from zero moments the first update is lr x sign(g) in every component)
    st[24:32] = g.uniform(0.5, 2.0, size=8) * 2e-3
    st[32:68] = 7.0   # stale camera fields and |tau|: every one is rewritten
    dtau = (g.normal(size=6) * 0.2).astype(np.float32)
    part = (g.normal(size=(n_part, 3)) * (0.5 / np.sqrt(n_part))).astype(np.float32)
    proj = np.zeros((4, 4), np.float32)
    proj[0, 0], proj[1, 1], proj[0, 2], proj[1, 2] = 1.3, 1.7, 0.02, -0.01
    proj[2, 2], proj[2, 3], proj[3, 2] = 1.0001, -0.010001, 1.0
    return st, dtau, part, proj.T.copy().reshape(-1)   # (the stored matrix is the transpose)


@functools.lru_cache(maxsize=None)
def pose_case(name):
    a_s, s_s, n_s = name.split("_")
    angle, step, n_part = float(a_s[1:]), int(s_s[1:]), int(n_s[1:])
    st, dtau, part, proj = _pose_inputs(step, n_part, 1000 * step + n_part)
    # the rotation update is linear in lr_rot: scale it to the angle asked for
    unit = pose_step(st, dtau, part, proj, (1.0, 0.0, 0.0), step, np.float64)[2]
    lr_rot = F32(angle / unit)
    lr = (lr_rot, F32(1e-6 if angle < 1e-4 else 1e-2), F32(0.01))
    o64, conv64, a64 = pose_step(st, dtau, part, proj, lr, step, np.float64)
    o32, conv32, _ = pose_step(st, dtau, part, proj, lr, step, np.float32)
    cam64 = pose_step(st, dtau, part, proj, lr, step, np.float64, camera_only=True)[0]
    cam32 = pose_step(st, dtau, part, proj, lr, step, np.float32, camera_only=True)[0]
    delta = MARGIN * abs(o32[67] - o64[67])
    return SimpleNamespace(name=name, angle=a64, step=step, n_part=n_part, st=st, dtau=dtau, part=part, proj=proj,
                           lr=lr, o64=o64, o32=o32, conv=conv64, conv_near=abs(o64[67] - POSE_CONV_TH) <= delta,
                           delta=delta, cam64=cam64, cam32=cam32)


def pose_check(c, got, conv, margin=None, o32=None):
    """``got``: the 68 floats after one step; ``conv``: the converged flag."""
    rep = Report("pose " + c.name)
    o32 = c.o32 if o32 is None else o32
    print(f"  DELTA |tau| {c.delta:.3e}; angle {c.angle:.3e}; converged decision {'near' if c.conv_near else 'clear'}")
    got = np.asarray(got, np.float64)
    for k, sl in POSE_GROUPS.items():
        _check(rep, "pose", k, got[sl], c.o64[sl], o32[sl], margin=margin)
    if got[14] != c.st[14] or got[15] != c.st[15]:
        rep.fails.append("pad floats 14, 15 were written")
    if conv is not None and not c.conv_near and int(conv) != c.conv:
        rep.fails.append(f"converged: {conv} against {c.conv}")
    return rep.finish()


def pose_check_camera(c, got, margin=None):
    """camera_only: R, T, the exposures and the moments keep their bits, the
    three camera fields are rebuilt."""
    rep = Report("pose camera_only " + c.name)
    got32 = np.asarray(got, np.float32)
    keepbits = np.r_[0:32, 67]
    if not np.array_equal(got32[keepbits].view(np.uint32), c.st[keepbits].view(np.uint32)):
        rep.fails.append("camera_only changed R, T, the exposures, the moments or |tau|")
    for k in ("viewmatrix", "projmatrix", "campos"):
        sl = POSE_GROUPS[k]
        _check(rep, "pose", k, got32[sl], c.cam64[sl], c.cam32[sl], margin=margin)
    return rep.finish()


# --------------------------------------------------------------------- DINO

DINO_K, DINO_TH, DINO_EPS = 128, 0.75, float(np.finfo(np.float32).eps)
# name -> (N, C, clusters, kind, _, what); dino_case picks each case's seed on the CPU
DINO_CASES = {
    "150x100": (150, 100, 1, "spread", 0, "VALU; C % 32 = 4: a partial last chunk"),
    "130x33": (130, 33, 1, "spread", 0, "VALU; one feature past a chunk"),
    "161x64": (161, 64, 1, "spread", 0, "MFMA at its smallest C"),
    "160x384": (160, 384, 1, "spread", 0, "MFMA at its largest C"),
    "300x448": (300, 448, 2, "spread", 0, "VALU past kSim2MaxC"),
    "96x768": (96, 768, 1, "spread", 0, "VALU, 24 chunks; N < K"),
    "60x16": (60, 16, 1, "spread", 0, "small N"),
    "3x16": (3, 16, 1, "spread", 0, "fewer rows than one selection workgroup holds"),
    "1x64": (1, 64, 1, "spread", 0, "a single sample, variance 0"),
    "64x64-apart": (64, 64, 0, "apart", 0, "every similarity below 0.75 off the diagonal: c = 1 in every row"),
}
# 96 samples stored twice (features and u bit-identical within a pair): every candidate value comes twice, so an
# even top_k cuts between two pairs in every row and an odd one inside a pair in every row -- both are run
DINO_TIE_K = (128, 127)
for _lay, _c, _w in (("adjacent", 64, "the pair adjacent"), ("far", 100, "the copies at j + 96: every pair straddles "
                                                                 "a 64-sample chunk boundary")):
    for _k in DINO_TIE_K:
        DINO_CASES[f"ties-{_lay}-k{_k}"] = (192, _c, 1, "ties-" + _lay, 0, "96 samples stored twice, " + _w)
DINO_PAD = tuple((n, c) for c in (64, 192, 384) for n in (33, 161))   # bit-identity of the two similarity kernels
for _n, _c in DINO_PAD:
    DINO_CASES[f"pad-{_n}x{_c}"] = (_n, _c, 1, "spread", 0, "k_dino_similarity2 against k_dino_similarity at C + 1")


def dino_inputs(N, C, clusters, kind, seed):
    g = torch.Generator().manual_seed(7919 * seed + 31 * N + C)
    if kind == "apart":
        feat = torch.randn(N, C, generator=g)
    else:
        n = 96 if kind.startswith("ties") else N
        centers = torch.randn(max(clusters, 1), C, generator=g)
        lo, hi = (0.05, 0.45) if kind.startswith("ties") else (0.05, 0.75)
        # a noise scale per sample: the similarities spread over (0.75, 1)
        s = lo + (hi - lo) * torch.rand(n, 1, generator=g)
        feat = centers[torch.randint(0, max(clusters, 1), (n,), generator=g)] + s * torch.randn(n, C, generator=g)
    u = 0.1 + 2.0 * torch.rand(feat.shape[0], generator=g)
    if kind == "ties-adjacent":
        feat, u = feat.repeat_interleave(2, 0), u.repeat_interleave(2)
    elif kind == "ties-far":
        feat, u = feat.repeat(2, 1), u.repeat(2)
    return feat.contiguous().numpy(), u.contiguous().numpy()


def dino_similarity(feat, dtype):
    """fn fn^T summed in k order, element by element (no BLAS blocking: bit-identical
    rows give bit-identical similarities, as they do in both kernels)."""
    x = feat.astype(dtype)
    n = np.maximum(np.sqrt((x * x).sum(1, dtype=dtype)), dtype(1e-12))
    fn = x / n[:, None]
    S = np.zeros((x.shape[0], x.shape[0]), dtype)
    for k in range(x.shape[1]):
        S += np.outer(fn[:, k], fn[:, k])
    return S


def dino_select(S, i, K=DINO_K, tooth=None):
    """The selected indices of row i: the candidates s > 0.75, and with more
    than K of them the K largest, ties at the K-th value in index order."""
    cand = np.flatnonzero(S[i] > DINO_TH)
    if cand.size > K:
        order = cand[np.argsort(-S[i][cand], kind="stable")]
        if tooth == "k_plus_1":
            return order[:K + 1]
        if tooth == "tie_twice":  # both copies of the pair the cut falls inside, the lowest other one dropped
            assert S[i][order[K - 1]] == S[i][order[K]]
            return np.r_[order[:K - 2], order[K - 1], order[K]]
        return order[:K]
    return cand


def dino_run(feat, u, dtype, K=DINO_K, S=None, tooth=None, tooth_row=None):
    """dino.hip's header in ``dtype`` -> dict(S, row_var, grad_u, loss, count)."""
    S = dino_similarity(feat, dtype) if S is None else S
    N = S.shape[0]
    u = u.astype(dtype)
    eps = dtype(DINO_EPS)
    row_var, grad, count = np.zeros(N, dtype), np.zeros(N, dtype), np.zeros(N, np.int64)
    for i in range(N):
        mine = tooth if i == tooth_row else None
        sel = dino_select(S, i, K, tooth=mine if mine in ("k_plus_1", "tie_twice") else None)
        c = dtype(sel.size)
        cn = c + eps
        us = u[sel]
        mean = us.sum(dtype=dtype) / cn
        d = us - mean
        row_var[i] = (d * d).sum(dtype=dtype) / (c if mine == "no_eps" else cn)
        count[i] = sel.size
        np.add.at(grad, sel, (dtype(2) * d - dtype(2) * d.sum(dtype=dtype) / cn) / cn * (dtype(1) / dtype(N)))
    loss = row_var.sum(dtype=dtype) / dtype(N)
    return dict(S=S.astype(np.float64), row_var=row_var.astype(np.float64), grad_u=grad.astype(np.float64),
                loss=np.float64(loss), count=count, row_var_bits=row_var.copy())


def dino_near_rows(S64, delta, K=DINO_K):
    """Near rows: a similarity within delta of the threshold, or with more than
    K candidates a gap under delta where the cut falls: between the K-th and
    the (K+1)-th largest candidate when they differ, and when they are equal
    (the cut inside a tie group, which any order resolves to the same
    uncertainties) between that value and the next distinct one on either side."""
    N = S64.shape[0]
    near = (np.abs(S64 - DINO_TH) <= delta).any(1)
    inside = np.zeros(N, bool)
    over = np.zeros(N, bool)
    for i in range(N):
        v = np.sort(S64[i][S64[i] > DINO_TH])[::-1]
        if v.size <= K:
            continue
        over[i] = True
        a, b = v[K - 1], v[K]
        if a != b:
            gap = a - b
        else:
            inside[i] = True
            above, below = v[v > a], v[v < a]
            gap = min(above.min() - a if above.size else np.inf, a - below.max() if below.size else np.inf)
        near[i] |= gap <= delta
    return near, over, inside


def dino_build(name, seed):
    N, C, clusters, kind, _, what = DINO_CASES[name]
    feat, u = dino_inputs(N, C, clusters, kind, seed)
    top_k = int(name.rsplit("-k", 1)[1]) if kind.startswith("ties") else DINO_K
    K = min(top_k, N)
    o64, o32 = dino_run(feat, u, np.float64, K), dino_run(feat, u, np.float32, K)
    delta = MARGIN * _dev(o32["S"], o64["S"])
    near, over, inside = dino_near_rows(o64["S"], delta, K)
    return SimpleNamespace(name=name, top_k=top_k, K=K, N=feat.shape[0], C=C, kind=kind, feat=feat, u=u, o64=o64,
                           o32=o32, delta=delta,
                           near=near, over=over, inside=inside, seed=seed, what=what)


def dino_needs(c):
    """What a seed has to offer beyond zero near rows."""
    if c.kind.startswith("ties"):
        return bool(c.over.all()) and bool(c.inside.all() if c.top_k % 2 else not c.inside.any())
    if c.name in ("150x100", "130x33", "161x64", "160x384", "300x448") or c.name.startswith("pad-161"):
        return bool(c.over.any()) and not bool(c.over.all())
    if c.name == "64x64-apart":
        return bool((c.o64["count"] == 1).all())
    return not bool(c.over.any())


@functools.lru_cache(maxsize=None)
def dino_case(name):
    for seed in range(64):   # the first seed whose float64 oracle alone has zero near rows and what the case needs
        c = dino_build(name, seed)
        if not c.near.any() and dino_needs(c):
            return c
    raise AssertionError(f"dino case {name}: no seed under 64 with zero near rows")


def dino_check(c, got, margin=None, tensors=("S", "row_var", "grad_u", "loss")):
    rep = Report("dino " + c.name)
    print(f"  DELTA similarity {c.delta:.3e}; {int(c.near.sum())} near rows of {c.N}; {int(c.over.sum())} rows "
          f"with more than K candidates, {int(c.inside.sum())} cut inside a tie")
    for k in tensors:
        _check(rep, "dino", k, got[k], c.o64[k], c.o32[k], margin=margin)
    if "row_var" in tensors:
        # a row that selects itself alone sums nothing: every operation is one
        # correctly rounded fp32 operation on the restatement's operands
        one = np.flatnonzero((c.o64["count"] == 1) & ~c.near)
        g = np.asarray(got["row_var"], np.float32)[one].view(np.uint32)
        want = c.o32["row_var_bits"][one].view(np.uint32)
        if not np.array_equal(g, want):
            rep.fails.append(f"row_var: {int((g != want).sum())} single-sample rows differ in bits from the fp32 "
                             "restatement")
    return rep.finish()


# ------------------------------------------------------ mapping: activations

MAP_P = (1, 255, 257, 1000)
MAP_IMAGES = ((1, 1), (7, 37), (16, 16), (33, 129))
QFLOOR = 1e-12
ISO_WEIGHTS = (0.0, "10/3P")


def act_inputs(P, seed=11):
    """Row 0 is generic; the special rows follow where P has room for them."""
    g = np.random.default_rng(seed + P)
    o = g.normal(size=P).astype(np.float32) * 2
    s = g.uniform(-9, 3, size=(P, 3)).astype(np.float32)
    q = g.normal(size=(P, 4)).astype(np.float32)
    special = {}
    if P > 16:
        o[1], o[2] = 20.0, -20.0
        s[3], s[4] = (-9, -9, 3), (3, -9, 3)
        s[5] = s[5, 0]                      # three bit-equal scales
        s[6] = 1.234
        s[7, 1] = s[7, 0]                   # two equal
        s[8, 2] = s[8, 0]
        q[9] = np.array([0.5, -0.5, 0.5, 0.5]) * 1e-20   # norm 1e-20: divides by the floor
        q[10] = 0.0                                      # a zero row
        q[P - 2] = np.array([3, -4, 0, 0]) * 2e-21
        special = dict(equal3=(5, 6), equal2=(7, 8), floor=(9, 10, P - 2))
    gr = np.random.default_rng(seed + 7 * P)
    grads = dict(g_op=gr.normal(size=P).astype(np.float32), g_sc=gr.normal(size=(P, 3)).astype(np.float32),
                 g_rot=gr.normal(size=(P, 4)).astype(np.float32))
    radii = gr.integers(-3, 40, size=P).astype(np.int32)
    radii[gr.random(P) < 0.3] = 0
    stats = dict(radii=radii, m2d=gr.normal(size=(P, 3)).astype(np.float32),
                 max_radii=gr.integers(0, 30, size=P).astype(np.float32),
                 accum=gr.uniform(0, 5, size=P).astype(np.float32),
                 denom=gr.integers(0, 9, size=P).astype(np.float32))
    return dict(o=o, s=s, q=q, **grads, **stats), special


def act_forward(v):
    """k_activate's header on torch tensors -> (opacity, scales, rotations, iso per row)."""
    # torch.sigmoid, whose backward is the kernel's g (1 - y) y: 1 - y cancels for a large raw opacity, in the
    # reference as in the kernel.  (Differentiating 1 / (1 + exp(-o)) through the reciprocal does not cancel; with
    # that restatement the spread of d_o's smallest group was 34 times under the kernel's error on MI355X.)
    op = torch.sigmoid(v["o"])
    e = torch.exp(v["s"])
    m = ((e[:, 0] + e[:, 1] + e[:, 2]) / 3.0)[:, None]
    iso = torch.abs(e - m).sum(1)
    return op, e, F.normalize(v["q"], dim=1, eps=QFLOOR), iso, e - m


def act_run(inp, iso_w, dtype, tooth=None):
    v = {k: torch.from_numpy(inp[k]).to(dtype) for k in ("o", "s", "q", "g_op", "g_sc", "g_rot")}
    for k in ("o", "s", "q"):
        v[k].requires_grad_(True)
    op, e, rot, iso, em = act_forward(v)
    if tooth == "no_projection":   # the normalise backward without the projection term
        n = v["q"].detach().norm(dim=1, keepdim=True).clamp_min(QFLOOR)
        rot_b = v["q"] / n
    else:
        rot_b = rot
    iso_b = iso
    if tooth == "no_sm":           # the isotropic term's - sm dropped: the row mean held constant
        m = ((e[:, 0] + e[:, 1] + e[:, 2]) / 3.0)[:, None].detach()
        iso_b = torch.abs(e - m).sum(1)
    L = (op * v["g_op"]).sum() + (e * v["g_sc"]).sum() + (rot_b * v["g_rot"]).sum() + iso_w * iso_b.sum()
    L.backward()
    gx, gy = torch.from_numpy(inp["m2d"][:, 0]).to(dtype), torch.from_numpy(inp["m2d"][:, 1]).to(dtype)
    vis = inp["radii"] > 0
    accum = torch.from_numpy(inp["accum"]).to(dtype) + torch.sqrt(gx * gx + gy * gy) * torch.from_numpy(vis).to(dtype)
    iso_part = wg_sums(iso.detach().numpy(), np.float64 if dtype == torch.float64 else np.float32)
    return dict(opacity=_np64(op), scales=_np64(e), rotations=_np64(rot), iso=_np64(iso), iso_part=iso_part,
                iso_sum=iso_part.sum(),   # (the partials of this precision, summed exactly)
                em=_np64(em), d_o=_np64(v["o"].grad), d_s=_np64(v["s"].grad),
                d_r=_np64(v["q"].grad), accum=_np64(accum))


@functools.lru_cache(maxsize=None)
def act_case(P, iso_kind):
    inp, special = act_inputs(P)
    iso_w = 0.0 if iso_kind == 0.0 else F32(10.0 / (3 * P))
    o64, o32 = act_run(inp, iso_w, torch.float64), act_run(inp, iso_w, torch.float32)
    delta = MARGIN * _dev(o32["em"], o64["em"])
    equal3 = (inp["s"][:, 0] == inp["s"][:, 1]) & (inp["s"][:, 1] == inp["s"][:, 2])
    near = _near0(o64["em"], o32["em"], delta).any(1) & ~equal3 & (iso_w != 0)
    floor = np.sqrt((inp["q"].astype(np.float64) ** 2).sum(1)) <= QFLOOR
    vis = inp["radii"] > 0
    stats = dict(max_radii=np.where(vis, np.maximum(inp["max_radii"], inp["radii"].astype(np.float32)),
                                    inp["max_radii"]),
                 denom=np.where(vis, inp["denom"] + np.float32(1), inp["denom"]))
    return SimpleNamespace(name=f"P{P}-iso{iso_kind}", P=P, iso_w=iso_w, inp=inp, special=special, o64=o64, o32=o32,
                           delta=delta, near=near, equal3=equal3, floor=floor, vis=vis, stats=stats)


def act_check_forward(c, got, margin=None):
    """``got``: opacity [P], scales [P, 3], rotations [P, 4], iso_part [blocks]."""
    rep = Report("activate " + c.name)
    for k in ("opacity", "scales", "rotations", "iso_part"):
        _check(rep, "activate", k, got[k], c.o64[k], c.o32[k], margin=margin)
    _check(rep, "activate", "iso_sum", np.asarray(got["iso_part"], np.float64).sum(), c.o64["iso_sum"],
           c.o32["iso_sum"], margin=margin)
    return rep.finish()


def act_check_backward(c, got, margin=None, o32=None):
    """``got``: d_o [P], d_s [P, 3], d_r [P, 4].  The rows under the quaternion
    floor (gradients of 1e12) are a tensor of their own."""
    rep = Report("activate_bwd " + c.name)
    o32 = c.o32 if o32 is None else o32
    print(f"  DELTA |e - m| {c.delta:.3e}; {int(c.near.sum())} of {c.P} rows excluded")
    _check(rep, "activate_bwd", "d_o", got["d_o"], c.o64["d_o"], o32["d_o"], margin=margin)
    keep = np.broadcast_to(~c.near[:, None], (c.P, 3))
    _check(rep, "activate_bwd", "d_s", got["d_s"], c.o64["d_s"], o32["d_s"], keep=keep, margin=margin)
    g = np.asarray(got["d_r"], np.float64).reshape(c.P, 4)
    for name, rows in (("d_r", ~c.floor), ("d_r floor rows", c.floor)):
        if rows.any():
            _check(rep, "activate_bwd", name, g[rows], c.o64["d_r"][rows], o32["d_r"][rows], margin=margin)
    return rep.finish()


# ------------------------------------------------------- mapping: rgbd loss

MAPLOSS_W = (F32(0.9 * 0.8), F32(0.1))   # w_rgb, w_depth as the caller folds them (already divided by the counts)
DEPTH_TH = F32(0.01)
_MAPLOSS_SEED = {(1, 1): 5, (7, 37): 6, (16, 16): 7, (33, 129): 8}


def maploss_frame(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    gt[:, :, : W // 5] = 0.002                              # under the rgb threshold
    ren = (gt + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gd = 0.5 + 3.0 * torch.rand(1, H, W, generator=g)
    gd[:, : (H + 2) // 4, W // 3:] = 0.004 * torch.rand(1, (H + 2) // 4, W - W // 3, generator=g)   # gt_depth <= 0.01
    if H * W == 1:
        gd[:] = 1.5
    dep = gd + 0.5 * torch.randn(1, H, W, generator=g)
    ssim = 1e-4 * torch.randn(3, H, W, generator=g)         # a random plane standing for the SSIM gradient
    return dict(gt=gt, ren=ren, gd=gd, dep=dep, ssim=ssim, ea=torch.tensor([-0.05]), eb=torch.tensor([0.02]))


def maploss_run(t, use_ssim, dtype):
    v = {k: x.to(dtype) for k, x in t.items()}
    for k in ("ren", "dep", "ea", "eb"):
        v[k] = v[k].clone().requires_grad_(True)
    ea = torch.exp(v["ea"])
    image_ab = ea * v["ren"] + v["eb"]
    gsum = (v["gt"][0] + v["gt"][1]) + v["gt"][2]
    m = (gsum > RGB_TH).to(dtype)[None]
    r = image_ab * m - v["gt"] * m
    l1 = torch.abs(r).sum(0)
    dm = (v["gd"] > DEPTH_TH).to(dtype)
    rd = v["dep"] * dm - v["gd"] * dm
    l1d = torch.abs(rd)[0]
    L = MAPLOSS_W[0] * l1.sum() + MAPLOSS_W[1] * l1d.sum()
    if use_ssim:
        L = L + (v["ssim"] * image_ab).sum()
    L.backward()
    ndt = np.float64 if dtype == torch.float64 else np.float32
    d_image = v["ren"].grad
    with torch.no_grad():   # per pixel: d/da = sum_c d_image x, d/db = sum_c d_image / exp(a)
        da_px = (d_image * v["ren"]).sum(0)
        db_px = (d_image / ea).sum(0)
    raw = lambda x: x.detach().numpy()  # noqa: E731
    part = dict(part_l1=wg_sums(raw(l1), ndt), part_l1d=wg_sums(raw(l1d), ndt), part_da=wg_sums(raw(da_px), ndt),
                part_db=wg_sums(raw(db_px), ndt))
    sums = {k.replace("part", "sum"): x.sum() for k, x in part.items()}   # (this precision's partials, summed exactly)
    return dict(image_ab=_np64(image_ab), d_image=_np64(d_image), d_depth=_np64(v["dep"].grad), **part, **sums,
                grad_ea=_np64(v["ea"].grad)[0], grad_eb=_np64(v["eb"].grad)[0],
                r=_np64(r), rd=_np64(rd)[0], gsum=_np64(gsum), m=_np64(m)[0], dm=_np64(dm)[0])


@functools.lru_cache(maxsize=None)
def maploss_case(H, W, use_ssim):
    t = maploss_frame(H, W, _MAPLOSS_SEED[(H, W)])
    o64, o32 = maploss_run(t, use_ssim, torch.float64), maploss_run(t, use_ssim, torch.float32)
    delta = dict(residual=MARGIN * _dev(o32["r"], o64["r"]), depth_residual=MARGIN * _dev(o32["rd"], o64["rd"]),
                 gt_sum=MARGIN * _dev(o32["gsum"], o64["gsum"]))
    # (gt_depth > 0.01 compares an input with a constant: the same in every precision)
    near = (_near0(o64["r"], o32["r"], delta["residual"]) & (o64["m"] != 0)[None]).any(0)
    near |= _near0(o64["rd"], o32["rd"], delta["depth_residual"]) & (o64["dm"] != 0)
    near |= np.abs(o64["gsum"] - RGB_TH) <= delta["gt_sum"]
    census = dict(rgb_mask=o64["m"] > 0, depth_mask=o64["dm"] > 0)
    near_wg = wg_sums(near.astype(np.float64)) > 0
    return SimpleNamespace(name=f"{H}x{W}-{'ssim' if use_ssim else 'l1'}", H=H, W=W, use_ssim=use_ssim, t=t, o64=o64,
                           o32=o32, delta=delta, near=near, near_wg=near_wg, census=census)


MAPLOSS_PIXEL = ("image_ab", "d_image", "d_depth")
MAPLOSS_PART = ("part_l1", "part_l1d", "part_da", "part_db")


def maploss_check(c, got, margin=None):
    """``got``: MAPLOSS_PIXEL as [3 or 1, H, W] and MAPLOSS_PART as [blocks]."""
    rep = Report("maploss " + c.name)
    print(f"  DELTA {c.delta}; {int(c.near.sum())} of {c.near.size} pixels excluded")
    for k in MAPLOSS_PIXEL:
        keep = None if k == "image_ab" else np.broadcast_to(~c.near, c.o64[k].shape)
        _check(rep, "maploss", k, got[k], c.o64[k], c.o32[k], keep=keep, margin=margin)
    for k in MAPLOSS_PART:
        exact = k in ("part_l1", "part_l1d")   # the L1 sums are continuous in the decisions
        _check(rep, "maploss", k, got[k], c.o64[k], c.o32[k], keep=None if exact else ~c.near_wg, margin=margin)
        if exact or not c.near.any():
            s = k.replace("part", "sum")
            _check(rep, "maploss", s, np.asarray(got[k], np.float64).sum(), c.o64[s], c.o32[s], margin=margin)
    return rep.finish()
