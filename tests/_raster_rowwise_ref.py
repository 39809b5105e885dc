"""Row-wise reference for the rasteriser's outputs and gradients: the cases,
the float64 oracle and fp32 restatement runs (cached per case) and the bound.

The bound is the derived form of tests/test_gpu_droid_ba.py:

    |got - oracle64| <= MARGIN * spread + 1e-6 * scale,
    spread = max |restatement32 - oracle64|,  scale = max |oracle64|,

the factor 8 standing for "another summation order".  It is applied
* element-wise, spread and scale being the tensor's maxima (every gradient
  tensor; colour, depth and opacity at the unmasked pixels; the summed pose
  gradient), and
* stratified: the rows that carry gradient are ordered by their largest
  float64 entry and cut into GROUPS groups of equal count, spread and scale
  being each group's maxima -- a wrong row whose gradient is small next to
  the tensor's largest fails here.  (A group maximum, because one row's own
  fp32 deviation is a single noisy sample.)

Masking.  Every pixel's backward is linear in that pixel's upstream
gradient, so dL/dcolour and dL/ddepth are zeroed at the oracle's *near
pixels* (a blend decision within DELTA of its threshold: alpha against
1/255, power against 0, T against 1e-4) for the GPU, the restatement and the
oracle alike: a threshold taken the other way there (__expf against expf
against float64 exp) changes no gradient.  *Near rows* (SH clamp, frustum
clamp, near cull within DELTA) are left out by row.  DELTA = 1e-4: a valid
alpha has power >= -5.6, which fp32 evaluates to a few 1e-6 relative, and T
is a product of at most a few hundred factors good to 2^-24 each; 1e-4
leaves more than 10 x over that.  At most MAX_MASKED of the pixels and
MAX_EXCLUDED of the rows that carry gradient may go this way
(tests/test_raster_rowwise_ref.py asserts it for every case).

Rows that are zero in the oracle (no pixel sends them gradient) must be
exactly zero; radii and num_rendered are exact.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from _util import GRAD_KEYS, load_scene, scene_names
from oracle import cpu_oracle, dense

DELTA = 1e-4
MARGIN = 8
# per-tensor margins above MARGIN, each with its cause and measurement
MARGINS: dict = {}
GROUPS = 8
MAX_MASKED = 0.01
MAX_EXCLUDED = 0.01
IMAGES = ("color", "depth", "opacity")

CASES = ("small", "wide", "saturated", "deep_tile", "precomp", "scalemod", "larger")


def _settings(W, H, view, deg, bg, scale_modifier=1.0):
    from wgsr.camera import synthetic_camera
    f = synthetic_camera(W, H, view).raster_fields()
    return dict(H=H, W=W, tanfovx=f["tanfovx"], tanfovy=f["tanfovy"], bg=torch.tensor(bg),
                scale_modifier=scale_modifier, viewmatrix=f["viewmatrix"], projmatrix=f["projmatrix"],
                projmatrix_raw=f["projmatrix_raw"], sh_degree=deg, campos=f["campos"])


def _scene_inputs(sc):
    return dict(means3D=sc.means3D, opacities=sc.opacities, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)


def _build(name):
    """(inputs, settings, (dL_dcolor, dL_ddepth)) of a synthetic case."""
    from wgsr.scene import make_scene, make_upstream_grads
    W, H = 72, 56  # 4.5 x 3.5 tiles: partial tiles right and bottom, partial bins at shift 1 and 2
    if name == "small":
        sc = make_scene(301, W, H, 3, seed=101)
        sc.shs[7:19, 0, :] = -2.5  # colours clamped at 0
        inputs, settings = _scene_inputs(sc), _settings(W, H, 2, 3, [0.3, 0.55, 0.8])
    elif name == "wide":
        sc = make_scene(200, W, H, 3, seed=102, log_scale_range=(math.log(0.02), math.log(0.3)))
        inputs, settings = _scene_inputs(sc), _settings(W, H, 1, 3, [0.1, 0.2, 0.3])
    elif name == "saturated":
        sc = make_scene(603, W, H, 1, seed=103, opacity_range=(0.6, 0.999),
                        log_scale_range=(math.log(0.15), math.log(0.6)))
        inputs, settings = _scene_inputs(sc), _settings(W, H, 0, 1, [1.0, 0.9, 0.8])
    elif name == "deep_tile":
        sc = make_scene(1501, W, H, 0, seed=104)
        g = torch.Generator().manual_seed(1104)
        z = sc.means3D[:, 2]
        # centres drawn into the 8 x 8 pixels around (40, 24), the middle of tile (2, 1)
        px = 36.0 + 8.0 * torch.rand(1501, generator=g)
        py = 20.0 + 8.0 * torch.rand(1501, generator=g)
        f = 0.9 * W
        sc.means3D[:, 0] = (px - W / 2) / f * z
        sc.means3D[:, 1] = (py - H / 2) / f * z
        inputs, settings = _scene_inputs(sc), _settings(W, H, 0, 0, [0.2, 0.4, 0.6])
    elif name == "precomp":
        sc = make_scene(301, W, H, 0, seed=105)
        g = torch.Generator().manual_seed(1105)
        R = dense.quat_to_rot(sc.rotations.double())
        Sig = R @ torch.diag_embed(sc.scales.double() ** 2) @ R.transpose(1, 2)
        cov6 = torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]],
                           dim=1).float().contiguous()
        inputs = dict(means3D=sc.means3D, opacities=sc.opacities, colors_precomp=torch.rand(301, 3, generator=g),
                      cov3D_precomp=cov6)
        settings = _settings(W, H, 1, 0, [0.3, 0.0, 0.7])
    elif name == "scalemod":
        sc = make_scene(301, W, H, 3, seed=106)
        inputs, settings = _scene_inputs(sc), _settings(W, H, 3, 1, [0.0, 0.5, 0.25], scale_modifier=1.7)
    elif name == "larger":
        W, H = 136, 104  # 8.5 x 6.5 tiles: 3 x 2 bins at shift 2, the right and bottom ones partial
        sc = make_scene(1500 + 3, W, H, 0, seed=107)
        inputs, settings = _scene_inputs(sc), _settings(W, H, 0, 0, [0.5, 0.25, 0.75])
    else:
        raise KeyError(name)
    seed = 1000 + CASES.index(name)
    return inputs, settings, make_upstream_grads(settings["W"], settings["H"], seed=seed)


def _restatement(inputs, settings, grads):
    cr = cpu_oracle.CpuRaster(**inputs, **settings)
    o32 = cr.backward(*grads)
    o32.update(color=cr.color, depth=cr.depth, opacity=cr.opacity, radii=cr.radii, num_rendered=cr.num_rendered)
    cr.close()
    return o32


def _np64(v):
    return v.numpy() if torch.is_tensor(v) else v


@functools.lru_cache(maxsize=None)
def case(name):
    """A synthetic case (CASES) or a committed golden scene ("golden:NAME"),
    with the float64 oracle and the fp32 restatement run once on the masked
    upstream gradients.  Treat every field as read-only."""
    if name.startswith("golden:"):
        # The float64 expectation comes from the file.  The file was made with
        # the unmasked upstream gradients, so a scene with near pixels takes
        # the masked expectation from a live run of the same oracle, after the
        # live unmasked run has reproduced the file to its float32 rounding.
        inputs, settings, expect, grads = load_scene(name[7:])
        rep = dense.dense_forward_backward(inputs, settings, *grads, near_delta=DELTA, mask_near=True)
        if bool(rep["near_pixels"].any()):
            full = dense.dense_forward_backward(inputs, settings, *grads)
            for k, v in expect.items():
                if isinstance(v, np.ndarray) and v.dtype.kind == "f":
                    np.testing.assert_allclose(v, _np64(full[k]).reshape(v.shape), rtol=2.0 ** -23, atol=1e-30,
                                               err_msg=f"{name} {k}: the live oracle against the file")
            o64 = {k: _np64(v) for k, v in rep.items()}
        else:
            o64 = {k: np.asarray(v, np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v
                   for k, v in expect.items()}
    else:
        inputs, settings, grads = _build(name)
        rep = dense.dense_forward_backward(inputs, settings, *grads, near_delta=DELTA, mask_near=True)
        o64 = {k: _np64(v) for k, v in rep.items()}
    far = ~rep["near_pixels"]
    grads = tuple((g * far).contiguous() for g in grads)
    o32 = _restatement(inputs, settings, grads)
    report = {k: _np64(rep[k]) for k in ("near_pixels", "near_rows", "stopped", "list_len", "rect", "sat_entries",
                                         "sh_clamped")}
    return SimpleNamespace(name=name, inputs=inputs, settings=settings, grads=grads, o64=o64, o32=o32,
                           near_pixels=report["near_pixels"], near_rows=report["near_rows"], report=report)


def grad_tensors(c):
    """The gradient tensors this case has a float64 expectation for."""
    return [k for k in GRAD_KEYS if c.o64.get(k) is not None and c.inputs.get(_INPUT_OF[k]) is not None]


_INPUT_OF = dict(dL_dmeans3D="means3D", dL_dmeans2D="means3D", dL_dopacity="opacities", dL_dsh="shs",
                 dL_dcolors="colors_precomp", dL_dscales="scales", dL_drotations="rotations",
                 dL_dcov3D="cov3D_precomp")


def rows_of(c, k, v):
    """[P, n] float64 view of gradient tensor k (dL_dsh: the whole table)."""
    P = c.inputs["means3D"].shape[0]
    return np.asarray(v, np.float64).reshape(P, -1)


def carrying(c, k):
    """Indices of the rows of tensor k that carry gradient in the oracle and
    are not near rows."""
    o = rows_of(c, k, c.o64[k])
    return np.flatnonzero(np.any(o != 0, axis=1) & ~c.near_rows)


def groups(c, k):
    """The carrying rows ordered by their largest float64 entry, cut into
    GROUPS groups of equal count (lowest magnitude first)."""
    rows = carrying(c, k)
    mag = np.abs(rows_of(c, k, c.o64[k])[rows]).max(1)
    return [g for g in np.array_split(rows[np.argsort(mag, kind="stable")], GROUPS) if g.size]


def _bound(what, got, o64, o32, margin, fails, ratios, key):
    err, spread, scale = np.abs(got - o64).max(), np.abs(o32 - o64).max(), np.abs(o64).max()
    ratio = err / spread if spread > 0 else (0.0 if err == 0 else np.inf)
    ratios[key] = max(ratios.get(key, 0.0), ratio)
    ok = err <= margin * spread + 1e-6 * scale
    print(f"  {what}: err {err:.3e} spread {spread:.3e} ratio {ratio:.2f} scale {scale:.3e}{'' if ok else '  FAIL'}")
    if not ok:
        fails.append(f"{what}: err {err:.3e} > {margin} * {spread:.3e} + 1e-6 * {scale:.3e}")


def check(c, got, margin=None):
    """Apply every check of this module to ``got`` (the dict of
    test_gpu_raster.run_c, numpy arrays).  Prints each err / spread ratio,
    raises AssertionError naming everything that failed, and returns the worst
    ratio per tensor ("<tensor>" element-wise, "<tensor>/rows" stratified)."""
    fails, ratios = [], {}
    m = lambda k: margin if margin is not None else MARGINS.get(k, MARGIN)  # noqa: E731
    print(f"{c.name}:")
    if got["num_rendered"] != c.o64["num_rendered"]:
        fails.append(f"num_rendered {got['num_rendered']} != {c.o64['num_rendered']}")
    if not np.array_equal(got["radii"], c.o64["radii"]):
        fails.append(f"radii differ at {np.flatnonzero(np.asarray(got['radii']) != c.o64['radii'])[:8]}")
    far = ~c.near_pixels
    if far.any():
        for k in IMAGES:
            sel = lambda v: np.asarray(v, np.float64)[:, far]  # noqa: E731
            _bound(k, sel(got[k]), sel(c.o64[k]), sel(c.o32[k]), m(k), fails, ratios, k)
    for k in grad_tensors(c):
        g, o64, o32 = (rows_of(c, k, v) for v in (got[k], c.o64[k], c.o32[k]))
        if g.shape != o64.shape:
            fails.append(f"{k}: shape {np.shape(got[k])} against {np.shape(c.o64[k])}")
            continue
        keep = ~c.near_rows
        if not keep.any():
            continue
        zero = keep & ~np.any(o64 != 0, axis=1)
        bad = np.flatnonzero(zero & np.any(g != 0, axis=1))
        if bad.size:
            fails.append(f"{k}: {bad.size} rows without gradient are not zero, first {bad[:8]}")
        if k == "dL_dsh":
            K = 3 * (c.settings["sh_degree"] + 1) ** 2
            if np.any(g[:, K:] != 0):
                fails.append(f"{k}: coefficients beyond the active degree are not zero")
        _bound(k, g[keep], o64[keep], o32[keep], m(k), fails, ratios, k)
        for i, rows in enumerate(groups(c, k)):
            _bound(f"{k} rows group {i} ({rows.size})", g[rows], o64[rows], o32[rows], m(k), fails, ratios,
                   k + "/rows")
    tau = lambda v: np.asarray(v, np.float64).reshape(-1, 6).sum(0)  # noqa: E731
    _bound("dL_dtau (summed)", tau(got["dL_dtau"]), tau(c.o64["dL_dtau"]), tau(c.o32["dL_dtau"]), m("dL_dtau"),
           fails, ratios, "dL_dtau")
    assert not fails, f"{c.name}: " + "; ".join(fails)
    return ratios


def golden_cases():
    return ["golden:" + n for n in scene_names()]
