"""Element-wise reference for the loss-side kernels (SSIM, the uncertainty
MLP, the uncertainty mapping loss): the cases, the float64 oracle and fp32
restatement runs (cached per case; treat every field as read-only) and the
bound.

The bound is the derived form of tests/test_gpu_droid_ba.py and
tests/_raster_rowwise_ref.py:

    |got - oracle64| <= MARGIN * spread + 1e-6 * scale,
    spread = max |restatement32 - oracle64|,  scale = max |oracle64|,

oracle64 and restatement32 being the same CPU formulas evaluated in float64
and in float32 on the test's own inputs, the factor 8 standing for "another
summation order".  It is applied
* element-wise, spread and scale being the tensor's maxima, and
* stratified: the elements are ordered by a key and cut into up to GROUPS
  groups of equal count (never fewer than MIN_GROUP elements: a group's
  spread is a maximum over its members because one element's own fp32
  deviation is a single noisy sample), spread and scale being each group's
  maxima -- a wrong element that is small next to the tensor's largest, or
  that sits where fp32 is exact while another region cancels, fails here.
  The key is the float64 magnitude, or for the SSIM tensors the oracle's
  window variance s11 + s22: the fp32 error of the derivative maps is set by
  the cancellation in E[x^2] - E[x]^2 against the C2 floor, so a flat patch
  (variance 0) has a spread hundreds of times a textured pixel's.

Decisions.
* MLP: the backward is linear in each row's upstream du.  A *near row* (the
  float64 oracle has a hidden pre-activation within MLP_DELTA = 1e-5 of 0: a
  ReLU that fp32 may take the other way; pre-activations are sums of up to
  384 O(0.1) terms, good to about 1e-6 in fp32) gets du = 0 for the GPU, the
  restatement and the oracle alike.  The forward u needs no masking.
* Uncertainty loss: nothing upstream to zero, so a pixel whose float64
  oracle puts a decision within UNC_DELTA = 1e-4 (relative to the threshold,
  absolute against a threshold of 0) of its threshold is excluded from the
  comparison (it must still be finite).  Full resolution: |residual| of the
  rgb or depth L1 near 0, gt.sum near the rgb threshold, ref near 0.01 or
  the depth threshold, ref near rendered + 1, the weight 0.5 / r^2 near 0.1.
  Feature resolution: small_opacity near 0.9, small_depth near the depth
  threshold, and for d_unc the uncertainty near its 0.1 clip.
At most MAX_MASKED of the rows / pixels may go this way
(tests/test_loss_elementwise_ref.py asserts it for every case).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ssim as osim
from oracle import uncertainty as ou

MARGIN = 8
# per-tensor margins above MARGIN ("<family>:<tensor>"), each with its cause
# and the ratio err / spread measured against the float64 oracle
MARGINS: dict = {}
GROUPS = 8
MIN_GROUP = 32
MAX_MASKED = 0.01
MLP_DELTA = 1e-5
UNC_DELTA = 1e-4


# ---------------------------------------------------------------- the bound

class Report:
    """Collects the failures and the worst err / bound per tensor of one check."""

    def __init__(self, name):
        self.name, self.fails, self.ratios = name, [], {}
        print(f"{name}:")

    def bound(self, what, got, o64, o32, margin, key):
        err, spread, scale = np.abs(got - o64).max(), np.abs(o32 - o64).max(), np.abs(o64).max()
        lim = margin * spread + 1e-6 * scale
        ratio = err / lim if lim > 0 else (0.0 if err == 0 else np.inf)
        self.ratios[key] = max(self.ratios.get(key, 0.0), ratio)
        ok = err <= lim
        print(f"  RATIO {self.name} {what}: err {err:.3e} spread {spread:.3e} scale {scale:.3e} "
              f"err/spread {err / spread if spread > 0 else float(err > 0):.2f} err/bound {ratio:.3f}"
              f"{'' if ok else '  FAIL'}")
        if not ok:
            self.fails.append(f"{what}: err {err:.3e} > {margin} * {spread:.3e} + 1e-6 * {scale:.3e}")

    def finish(self):
        assert not self.fails, f"{self.name}: " + "; ".join(self.fails)
        return self.ratios


def strata(key):
    """Index groups of equal count, ordered by ``key`` (lowest first)."""
    key = np.asarray(key).reshape(-1)
    n = min(GROUPS, max(1, key.size // MIN_GROUP))
    return [g for g in np.array_split(np.argsort(key, kind="stable"), n) if g.size]


def check_tensor(rep, name, got, o64, o32, key=None, keep=None, margin=None, family=""):
    """Both forms of the bound on one tensor.  ``key``: the stratification key
    (default |o64|); ``keep``: bool mask of the elements compared (every
    element of ``got`` must be finite all the same)."""
    got, o64, o32 = (np.asarray(v, np.float64).reshape(-1) for v in (got, o64, o32))
    if got.shape != o64.shape:
        rep.fails.append(f"{name}: {got.size} elements against {o64.size}")
        return
    if not np.all(np.isfinite(got)):
        rep.fails.append(f"{name}: {np.count_nonzero(~np.isfinite(got))} elements are not finite")
        return
    key = np.abs(o64) if key is None else np.asarray(key, np.float64).reshape(-1)
    if keep is not None:
        keep = np.asarray(keep, bool).reshape(-1)
        got, o64, o32, key = got[keep], o64[keep], o32[keep], key[keep]
    if got.size == 0:
        return
    m = margin if margin is not None else MARGINS.get(f"{family}:{name}", MARGIN)
    rep.bound(name, got, o64, o32, m, name)
    gr = strata(key)
    if len(gr) > 1:
        for i, g in enumerate(gr):
            rep.bound(f"{name} group {i} ({g.size})", got[g], o64[g], o32[g], m, name + "/groups")


# --------------------------------------------------------------------- SSIM

SSIM_WINDOWS = (3, 5, 7, 9, 11)
SSIM_SHAPES = ((1, 16, 64),      # exactly one tile
               (1, 17, 65),      # one pixel into the next tile both ways: the halo crosses the seam
               (3, 33, 129),     # three tile columns, partial last tiles, plane offsets
               (1, 5, 4),        # smaller than the window
               (1, 1, 1),
               (2, 3, 35, 70))   # size_average=False with per-image weights
SSIM_KINDS = ("textured", "flat")
SSIM_WEIGHTS = (0.3, -2.0)       # per-image dL/dmean of the batch case: a wrong plane_scale index shows
SSIM_TENSORS = ("grad", "dmap0", "dmap1", "dmap2", "plane_mean")


def ssim_case_names():
    return [f"{'x'.join(map(str, s))}-w{ws}-{kind}" for s in SSIM_SHAPES for ws in SSIM_WINDOWS for kind in SSIM_KINDS]


def _ssim_images(shape, ws, kind):
    """(rendered, gt).  ``textured`` is the suite's pair (tests/test_gpu_ssim.py
    _pair); ``flat`` adds what the product renders and where C and D sit at
    their C1 / C2 floors: a constant patch present in both images, a black
    border in gt (the region rgb_boundary_threshold masks out) and a patch
    saturated at 1."""
    g = torch.Generator().manual_seed(sum(shape) + ws)
    gt = torch.rand(*shape, generator=g)
    ren = (gt + 0.08 * torch.randn(*shape, generator=g)).clamp(0, 1)
    if kind == "flat":
        H, W = shape[-2:]
        b = max(1, min(H, W) // 8)
        dark = 0.02 * torch.rand(*shape, generator=g)
        for sl in ((slice(0, b), slice(None)), (slice(H - b, H), slice(None)), (slice(None), slice(0, b)),
                   (slice(None), slice(W - b, W))):
            gt[(..., *sl)] = 0.0
            ren[(..., *sl)] = dark[(..., *sl)]
        # (12 rows of a 33-row frame: an 11-tap window fits inside.  The middle
        # columns, the tile seam of the wide frames, stay textured: where both
        # images agree over a whole window SSIM is at its maximum and there is
        # no gradient to get wrong)
        rows = slice(H // 4, H // 4 + 3 * H // 8)
        gt[..., rows, W // 8:3 * W // 8] = 0.5
        ren[..., rows, W // 8:3 * W // 8] = 0.5
        gt[..., rows, 5 * W // 8:7 * W // 8] = 1.0
        ren[..., rows, 5 * W // 8:7 * W // 8] = 1.0
    return ren.contiguous(), gt.contiguous()


def ssim_loss(val, weights):
    """The scalar the gradient is taken of: 1 - mean SSIM, or the weighted sum
    of the per-image means."""
    return 1.0 - val if weights is None else (val * weights.to(val)).sum()


def _ssim_grad(ren, gt, ws, weights, dtype):
    x = ren.to(dtype).clone().requires_grad_(True)
    ssim_loss(osim.ssim_torch(x, gt.to(dtype), ws, size_average=weights is None), weights).backward()
    return x.grad.numpy().astype(np.float64)


def _conv_same(plane, w2d, dtype):
    """oracle.ssim.conv_same in ``dtype`` (the same taps in the same order)."""
    ws = w2d.shape[0]
    r = ws // 2
    H, W = plane.shape
    p = np.zeros((H + 2 * r, W + 2 * r), dtype)
    p[r:r + H, r:r + W] = plane
    out = np.zeros((H, W), dtype)
    for i in range(ws):
        for j in range(ws):
            out += dtype(w2d[i, j]) * p[i:i + H, j:j + W]
    return out


def ssim_stats(x, y, ws, dtype, w2d=None):
    """oracle.ssim._stats in ``dtype`` (float64: that function itself), with
    an optional substitute window (the decisiveness test's dropped tap)."""
    if dtype is np.float64 and w2d is None:
        return osim._stats(x, y, ws)
    w = osim.window_2d(ws) if w2d is None else w2d
    x, y = x.astype(dtype), y.astype(dtype)
    mu1, mu2 = _conv_same(x, w, dtype), _conv_same(y, w, dtype)
    s11 = _conv_same(x * x, w, dtype) - mu1 * mu1
    s22 = _conv_same(y * y, w, dtype) - mu2 * mu2
    s12 = _conv_same(x * y, w, dtype) - mu1 * mu2
    return mu1, mu2, s11, s22, s12


def ssim_maps(stats, dtype):
    """The SSIM map and k_ssim_fwd's three derivative maps dS/dmu1,
    dS/dE[x^2], dS/dE[xy] (the formulas in its comment) from window
    statistics, in ``dtype``."""
    mu1, mu2, s11, s22, s12 = stats
    C1, C2, two = dtype(osim.C1), dtype(osim.C2), dtype(2)
    A, B = two * mu1 * mu2 + C1, two * s12 + C2
    C, D = mu1 * mu1 + mu2 * mu2 + C1, s11 + s22 + C2
    S = (A * B) / (C * D)
    d0 = two * mu2 * (B - A) / (C * D) - two * mu1 * S * (dtype(1) / C - dtype(1) / D)
    return S, np.stack([d0, -S / D, two * A / (C * D)])


def _ssim_forward(ren, gt, ws, dtype):
    """-> (dmap [3, planes, H, W], plane means [planes], s11 + s22 [planes, H, W])."""
    a = ren.numpy().reshape(-1, *ren.shape[-2:])
    b = gt.numpy().reshape(-1, *gt.shape[-2:])
    dmap, mean, var = [], [], []
    for p in range(a.shape[0]):
        st = ssim_stats(a[p], b[p], ws, dtype)
        S, d = ssim_maps(st, dtype)
        dmap.append(d)
        mean.append(S.mean(dtype=dtype))
        var.append(st[2] + st[3])
    return np.stack(dmap, 1).astype(np.float64), np.asarray(mean, np.float64), np.stack(var).astype(np.float64)


@functools.lru_cache(maxsize=None)
def ssim_case(name):
    shape_s, ws_s, kind = name.split("-")
    shape, ws = tuple(int(v) for v in shape_s.split("x")), int(ws_s[1:])
    ren, gt = _ssim_images(shape, ws, kind)
    weights = torch.tensor(SSIM_WEIGHTS, dtype=torch.float64) if len(shape) == 4 else None
    o = {}
    for tag, tdt, ndt in (("o64", torch.float64, np.float64), ("o32", torch.float32, np.float32)):
        dmap, mean, var = _ssim_forward(ren, gt, ws, ndt)
        o[tag] = dict(grad=_ssim_grad(ren, gt, ws, weights, tdt).reshape(var.shape), dmap0=dmap[0], dmap1=dmap[1],
                      dmap2=dmap[2], plane_mean=mean)
        if tag == "o64":
            key = var
    return SimpleNamespace(name=name, shape=shape, ws=ws, kind=kind, ren=ren, gt=gt, weights=weights, var=key,
                           o64=o["o64"], o32=o["o32"])


def ssim_check(c, got, margin=None):
    """``got``: dict of SSIM_TENSORS (grad and dmap* as [planes, H, W])."""
    rep = Report("ssim " + c.name)
    for k in SSIM_TENSORS:
        check_tensor(rep, k, got[k], c.o64[k], c.o32[k], key=None if k == "plane_mean" else c.var, margin=margin,
                     family="ssim")
    return rep.finish()


# ---------------------------------------------------------------------- MLP

def torch_mlp(net, x, masks=None, p=0.0):
    """MLPNetwork.forward with explicit dropout masks (torch's dropout:
    x * mask / (1 - p))."""
    H, W, C = x.shape[-3:]
    y = x.reshape(-1, C)
    for i, layer in enumerate(net.layers):
        y = F.relu(F.linear(y, layer.weight, layer.bias))
        if masks is not None:
            y = y * masks[i] * (1.0 / (1.0 - p))
    y = F.softplus(F.linear(y, net.output_layer.weight, net.output_layer.bias))
    return y.view(x.shape[:-1])


MLP_PARAMS = ("dW1", "db1", "dW2", "db2", "dW3", "db3")
# name -> (N, C, p, misaligned, the kernels its shape and alignment select)
MLP_CASES = {
    "1275x384": (1275, 384, 0.2, False, "k_mlp_fwd_small<384>, k_mlp_bwd2: partial 16- and 64-row blocks"),
    "17x64": (17, 64, 0.5, False, "k_mlp_fwd_small<64>, k_mlp_bwd2: one partial block"),
    "1x64": (1, 64, 0.0, False, "the single row"),
    "300x256": (300, 256, 0.2, False, "k_mlp_fwd_small<256>"),
    "1000x192": (1000, 192, 0.2, False, "k_mlp_fwd<16> by its natural route"),
    "65600x64": (65600, 64, 0.2, False, "k_mlp_fwd<64> (1025 workgroups), k_mlp_bwd (nb = 1025), 65 reduce segments"),
    "1275x384-offset4": (1275, 384, 0.2, True, "k_mlp_fwd<16>, k_mlp_bwd: the VALU kernels on the mapper's shape"),
}
MLP_SEG2 = ("1275x384", "300x384", (1.0, 0.5))   # forward_raw2 / backward_raw2, and the accumulate form
_MLP_EXTRA = {"300x384": (300, 384, 0.2, False, "the second segment")}


def _mlp_net(ws, dtype):
    w = [t.to(dtype).clone().requires_grad_(True) for t in ws]
    net = SimpleNamespace(layers=[SimpleNamespace(weight=w[0], bias=w[1]), SimpleNamespace(weight=w[2], bias=w[3])],
                          output_layer=SimpleNamespace(weight=w[4], bias=w[5]))
    return net, w


def mlp_run(c, dtype, du=None):
    """The oracle formulas in ``dtype``: -> dict(u, dW1 .. db3) as float64 numpy."""
    net, w = _mlp_net(c.weights, dtype)
    masks = None if c.p == 0 else [m.to(dtype) for m in c.masks]
    u = torch_mlp(net, c.x.to(dtype).view(1, c.N, c.C), masks, c.p).view(-1)
    (u * (c.du if du is None else du).to(dtype)).sum().backward()
    out = {k: t.grad.numpy().astype(np.float64) for k, t in zip(MLP_PARAMS, w)}
    out["u"] = u.detach().numpy().astype(np.float64)
    return out


@functools.lru_cache(maxsize=None)
def mlp_case(name):
    from wgsr.mlp import dropout_mask
    N, C, p, misaligned, what = {**MLP_CASES, **_MLP_EXTRA}[name]
    g = torch.Generator().manual_seed(1000 + N + C)
    ws = [torch.randn(64, C, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1,
          torch.randn(64, 64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1,
          torch.randn(1, 64, generator=g) * 0.1, torch.randn(1, generator=g) * 0.1]
    x = torch.randn(N, C, generator=g)
    du = torch.randn(N, generator=g)
    seed = 12345 + N
    masks = [torch.from_numpy(dropout_mask(seed, i, N, p)) for i in range(2)]
    # near rows: a hidden pre-activation of the float64 oracle within MLP_DELTA of 0
    xd, wd = x.double(), [t.double() for t in ws]
    z1 = xd @ wd[0].T + wd[1]
    h1 = F.relu(z1) * (masks[0].double() / (1.0 - p) if p > 0 else 1.0)
    z2 = h1 @ wd[2].T + wd[3]
    near = ((z1.abs() <= MLP_DELTA).any(1) | (z2.abs() <= MLP_DELTA).any(1)).numpy()
    du = (du * torch.from_numpy(~near)).contiguous()
    c = SimpleNamespace(name=name, N=N, C=C, p=p, misaligned=misaligned, what=what, weights=ws, x=x, du=du,
                        seed=seed, masks=masks, near=near)
    c.o64, c.o32 = mlp_run(c, torch.float64), mlp_run(c, torch.float32)
    return c


@functools.lru_cache(maxsize=None)
def mlp_seg2_case():
    """Two segments through one network (the first case's weights): u is the
    two forwards side by side, the gradient the sum of scale_i x backward_i."""
    a, b0 = mlp_case(MLP_SEG2[0]), mlp_case(MLP_SEG2[1])
    b = SimpleNamespace(**{**vars(b0), "weights": a.weights})
    # (other weights: b's near rows are taken again, on top of its own)
    xd, wd = b.x.double(), [t.double() for t in a.weights]
    z1 = xd @ wd[0].T + wd[1]
    z2 = (F.relu(z1) * b.masks[0].double() / (1.0 - b.p)) @ wd[2].T + wd[3]
    b.near = ((z1.abs() <= MLP_DELTA).any(1) | (z2.abs() <= MLP_DELTA).any(1)).numpy()
    b.du = (b0.du * torch.from_numpy(~b.near)).contiguous()
    s1, s2 = MLP_SEG2[2]
    o = {}
    for tag, dt in (("o64", torch.float64), ("o32", torch.float32)):
        ra = a.o64 if tag == "o64" else a.o32
        rb = mlp_run(b, dt)
        o[tag] = {k: s1 * ra[k] + s2 * rb[k] for k in MLP_PARAMS}
        o[tag]["u"] = np.concatenate([ra["u"], rb["u"]])
    return SimpleNamespace(name="seg2 " + "+".join(MLP_SEG2[:2]), a=a, b=b, scales=(s1, s2), o64=o["o64"], o32=o["o32"],
                           near=np.concatenate([a.near, b.near]))


def mlp_check(c, got, margin=None, tensors=("u",) + MLP_PARAMS):
    rep = Report("mlp " + c.name)
    for k in tensors:
        check_tensor(rep, k, got[k], c.o64[k], c.o32[k], margin=margin, family="mlp")
    return rep.finish()


def mlp_split_grad(flat, C):
    """The flat gradient of backward_raw (the parameters' order) -> dict."""
    flat = np.asarray(flat)
    sizes = (64 * C, 64, 64 * 64, 64, 64, 1)
    out, o = {}, 0
    for k, n in zip(MLP_PARAMS, sizes):
        out[k] = flat[o:o + n]
        o += n
    return out


# -------------------------------------------------- uncertainty mapping loss

# name -> (H, W, h, w, train_frac, ssim_frac, initialization, seed)
UNC_CASES = {
    "75x141-default": (75, 141, 5, 10, 0.3, 0.3, False, 3),
    "75x141-late": (75, 141, 5, 10, 0.9, 0.1, False, 9),
    "96x128-init": (96, 128, 7, 9, 0.3, 0.3, True, 5),
    "64x64-3x3": (64, 64, 3, 3, 0.3, 0.3, False, 7),
}
UNC_FULL = ("d_image", "d_depth")
UNC_SMALL = ("d_unc", "uncertainty_loss")
UNC_SCALARS = ("loss", "d_exposure_a", "d_exposure_b")
UNC_INPUTS = ("gt", "ren", "ref", "dep", "opa", "unc", "ea", "eb")


def unc_frame(H, W, h, w, seed):
    """tests/test_gpu_uncer.py's _frame scaled down (CPU tensors): the zero
    patch in gt, the zero and 90.0 patches in ref and the 0.05 entries in unc,
    so every mask has both outcomes."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    gt[:, :H // 8, :W // 8] = 0.0
    ren = (gt + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    ref = 1.0 + 3.0 * torch.rand(1, H, W, generator=g)
    ref[:, H // 5:H // 4, W // 5:W // 3] = 0.0
    ref[:, -(H // 3):, -(W // 3):] = 90.0
    dep = ref + 1.5 * torch.randn(1, H, W, generator=g)
    opa = torch.rand(1, H, W, generator=g) * 0.3 + 0.7
    unc = torch.rand(h, w, generator=g) * 2.5
    unc[0, :5] = 0.05
    ea = 0.05 * torch.randn(1, generator=g)
    eb = 0.02 * torch.randn(1, generator=g)
    return dict(gt=gt, ren=ren, ref=ref, dep=dep, opa=opa, unc=unc, ea=ea, eb=eb)


def unc_run(t, tf, sf, init, dtype):
    """oracle.uncertainty.loss_mapping_uncertainty and its autograd gradients
    in ``dtype`` -> dict of float64 numpy (exposure gradients None with
    ``init``: there is no exposure term)."""
    v = {k: x.to(dtype) for k, x in t.items()}
    for k in ("ren", "dep", "unc", "ea", "eb"):
        v[k] = v[k].clone().requires_grad_(True)
    loss = ou.loss_mapping_uncertainty(ou.DEFAULT_CONFIG, v["ren"], v["dep"], v["gt"], v["ref"], v["ea"], v["eb"],
                                       v["opa"], v["unc"], tf, sf, initialization=init)
    loss.backward()
    with torch.no_grad():
        img = v["ren"] if init else torch.exp(v["ea"]) * v["ren"] + v["eb"]
        H, W = v["gt"].shape[-2:]
        mask = (v["gt"].sum(dim=0) > ou.DEFAULT_CONFIG["Training"]["rgb_boundary_threshold"]).view(1, H, W)
        ul, ru, rgb_l1, depth_l1 = ou.mapping_loss_components(v["gt"], img, v["ref"], v["dep"], v["unc"], v["opa"],
                                                              tf, sf, ou.DEFAULT_CONFIG["uncertainty_params"], mask)
    np64 = lambda x: None if x is None else x.detach().numpy().astype(np.float64)  # noqa: E731
    return dict(loss=np64(loss), d_image=np64(v["ren"].grad), d_depth=np64(v["dep"].grad), d_unc=np64(v["unc"].grad),
                d_exposure_a=np64(v["ea"].grad), d_exposure_b=np64(v["eb"].grad), uncertainty_loss=np64(ul),
                ru=np64(ru), rgb_l1=np64(rgb_l1), depth_l1=np64(depth_l1), mask=mask.numpy())


def _near(x, thr):
    thr = np.asarray(thr, np.float64)
    return np.abs(x - thr) <= UNC_DELTA * np.where(thr == 0, 1.0, np.abs(thr))


def _unc_decisions(t, o64):
    """-> (full-resolution near pixels [H, W], feature-resolution near pixels
    for ul [h, w], the same plus the clip for d_unc, and a census of each
    mask's two outcomes) from the float64 oracle."""
    cfg, ucfg = ou.DEFAULT_CONFIG, ou.DEFAULT_CONFIG["uncertainty_params"]
    gt, ref, dep = t["gt"].double().numpy(), t["ref"].double().numpy()[0], t["dep"].double().numpy()[0]
    H, W = ref.shape
    thr_rgb = cfg["Training"]["rgb_boundary_threshold"]
    thr_depth = min(10 * float(t["ref"].double().median()), 50)
    mask = o64["mask"][0]
    dmask = (ref > 0.01) & (ref < thr_depth)
    weight = 0.5 / o64["ru"] ** 2
    near = (_near(o64["rgb_l1"], 0.0) & mask[None]).any(0)
    near |= _near(o64["depth_l1"][0], 0.0) & dmask
    near |= _near(gt.sum(0), thr_rgb)
    near |= _near(ref, 0.01) | _near(ref, thr_depth)
    near |= _near(ref, dep + 1.0)
    near |= _near(weight, 0.1)
    shape = t["unc"].shape
    small_op = ou._resample(t["opa"].double().view(H, W), shape).numpy()
    small_depth = ou._resample(t["ref"].double().squeeze(), shape, "bicubic").numpy()
    near_small = _near(small_op, ucfg["opacity_th_for_uncer_loss"]) | _near(small_depth, thr_depth)
    near_clip = near_small | _near(t["unc"].double().numpy(), 0.1)
    census = dict(rgb_mask=mask, depth_mask=dmask, under=ref < dep + 1.0, weight_cut=weight < 0.1,
                  small_opacity=small_op < ucfg["opacity_th_for_uncer_loss"], small_depth=small_depth > thr_depth,
                  clip=t["unc"].numpy() < 0.1)
    return near, near_small, near_clip, census


@functools.lru_cache(maxsize=None)
def unc_case(name):
    H, W, h, w, tf, sf, init, seed = UNC_CASES[name]
    t = unc_frame(H, W, h, w, seed)
    o64, o32 = unc_run(t, tf, sf, init, torch.float64), unc_run(t, tf, sf, init, torch.float32)
    near, near_small, near_clip, census = _unc_decisions(t, o64)
    return SimpleNamespace(name=name, t=t, tf=tf, sf=sf, init=init, o64=o64, o32=o32, near=near,
                           near_small=near_small, near_clip=near_clip, census=census)


def unc_check(c, got, margin=None):
    """``got``: dict of UNC_FULL + UNC_SMALL + UNC_SCALARS (numpy)."""
    rep = Report("uncer " + c.name)
    far = ~c.near
    for k in UNC_FULL:
        keep = np.broadcast_to(far, c.o64[k].shape)
        check_tensor(rep, k, got[k], c.o64[k], c.o32[k], keep=keep, margin=margin, family="uncer")
    check_tensor(rep, "d_unc", got["d_unc"], c.o64["d_unc"], c.o32["d_unc"], keep=~c.near_clip, margin=margin,
                 family="uncer")
    check_tensor(rep, "uncertainty_loss", got["uncertainty_loss"], c.o64["uncertainty_loss"],
                 c.o32["uncertainty_loss"], keep=~c.near_small, margin=margin, family="uncer")
    for k in UNC_SCALARS:
        if c.o64[k] is not None:
            check_tensor(rep, k, got[k], c.o64[k], c.o32[k], margin=margin, family="uncer")
    return rep.finish()
