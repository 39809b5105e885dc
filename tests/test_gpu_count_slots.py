"""The forward's counter block: k_preprocess's waves add their pair counts and
depth-key maxima into kCountSlots 64-byte records (slot = workgroup %
kCountSlots, csrc/wgsr_common.h), and every reader reduces the slots: the
scan's first wave (the published counts and the header the host's copy paths
read), k_cap_counts (capacity mode) and the Gaussian-level depth sort's key
range.

Sizes around the slot wrap (fewer workgroups than slots, one each, reused
slots), everything culled, the schedules and count paths against each other,
a key range whose extremes sit in different slots, a small forward right
after a large one (no stale slots) and capacity mode.  160 x 120 frames, SH0
scenes from wgsr.scene.make_scene; counts against the CPU oracle exactly.
"""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W, H = 160, 120
NAMES = ("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations", "tau")


def _slots():
    """The committed slot count, from the source the library is built from."""
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    src = open(os.path.join(root, "wildgs-slam-blackwell_amd", "csrc", "wgsr_common.h")).read()
    return int(re.search(r"constexpr int kCountSlots = (\d+);", src).group(1))


S = _slots()
P_WRAP = 64 * S + 65  # every slot used once, then one more round on the first two


def _cam():
    from wgsr.camera import synthetic_camera
    return synthetic_camera(W, H, 0).raster_fields()


@functools.lru_cache(maxsize=None)
def _scene(P, kind="plain"):
    from wgsr.scene import make_scene
    sc = make_scene(P, W, H, 0, seed=11)
    means = sc.means3D
    if kind == "behind":  # every Gaussian behind the camera
        means = means * torch.tensor([1.0, 1.0, -1.0])
    elif kind == "range":  # depths 0.3 .. 1e4 in index order, screen positions kept
        z = torch.exp(torch.linspace(math.log(0.3), math.log(1e4), P, dtype=torch.float64)).float()
        means = means * (z / means[:, 2]).unsqueeze(1)
        means[:, 2] = z
    return means.contiguous(), sc.opacities, sc.scales, sc.rotations, sc.shs


def _oracle(scene):
    from oracle import cpu_oracle
    means, opac, scales, rots, shs = scene
    f = _cam()
    return cpu_oracle.CpuRaster(means3D=means, opacities=opac, shs=shs, scales=scales, rotations=rots, H=H, W=W,
                                tanfovx=f["tanfovx"], tanfovy=f["tanfovy"], bg=torch.zeros(3), scale_modifier=1.0,
                                viewmatrix=f["viewmatrix"], projmatrix=f["projmatrix"],
                                projmatrix_raw=f["projmatrix_raw"], sh_degree=0, campos=f["campos"])


def _run(scene, backward=True, bg=(0.0, 0.0, 0.0)):
    """One forward (+ backward) through the C ABI: every output as numpy."""
    from diff_gaussian_rasterization import _C
    from wgsr.scene import make_upstream_grads
    f = _cam()
    d = lambda x: x.to(DEV).contiguous()  # noqa: E731
    means, opac, scales, rots, shs = (d(x) for x in scene)
    e = torch.empty(0, device=DEV)
    bgt = d(torch.tensor(bg))
    cam = [d(f["viewmatrix"]), d(f["projmatrix"]), d(f["projmatrix_raw"])]
    nr, color, radii, geom, binning, img, depth, opacity, nt = _C.rasterize_gaussians(
        bgt, means, e, opac, scales, rots, 1.0, e, *cam, f["tanfovx"], f["tanfovy"], H, W, shs, 0, d(f["campos"]),
        False, False)
    res = dict(num_rendered=nr, color=color, depth=depth, opacity=opacity, radii=radii, n_touched=nt)
    if backward:
        gc, gd = make_upstream_grads(W, H, seed=6)
        grads = _C.rasterize_gaussians_backward(bgt, means, radii, e, scales, rots, 1.0, e, *cam, f["tanfovx"],
                                                f["tanfovy"], d(gc), d(gd), shs, 0, d(f["campos"]), geom, nr,
                                                binning, img, False)
        res.update({"dL_d" + k: g for k, g in zip(NAMES, grads)})
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def _same(a, b, tag):
    assert a.keys() == b.keys()
    for k, v in a.items():
        if k == "num_rendered":
            assert b[k] == v, tag
        else:
            np.testing.assert_array_equal(b[k], v, err_msg=f"{tag}: {k}")


@functools.lru_cache(maxsize=None)
def _default(P, kind="plain"):
    """The default path's outputs of a scene, computed once."""
    for k in ("WGSR_PUBLISH_COUNTS", "WGSR_DEPTH_SORT", "WGSR_BIN_DEPTH_MAX_AVG"):
        assert k not in os.environ
    return _run(_scene(P, kind))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 64 * S - 1, 64 * S, P_WRAP])
def test_counts_match_the_oracle_around_the_slot_wrap(P):
    scene = _scene(P)
    out = _run(scene, backward=False)
    cr = _oracle(scene)
    assert out["num_rendered"] == cr.num_rendered
    np.testing.assert_array_equal(out["radii"], cr.radii)
    if P >= 63:
        assert out["num_rendered"] > 0


def test_all_culled():
    bg = (0.1, 0.2, 0.3)
    out = _run(_scene(P_WRAP, "behind"), bg=bg)
    assert out["num_rendered"] == 0
    assert not out["radii"].any()
    np.testing.assert_array_equal(out["color"], np.broadcast_to(np.float32(bg)[:, None, None], (3, H, W)))
    for k in NAMES:
        assert not out["dL_d" + k].any(), k


@pytest.mark.parametrize("env", [
    {"WGSR_PUBLISH_COUNTS": "0"},      # the header copied behind the scan
    {"WGSR_DEPTH_SORT": "global"},     # the whole block copied ahead of the depth sort; the range from the slots
    {"WGSR_DEPTH_SORT": "full"},
    {"WGSR_BIN_DEPTH_MAX_AVG": "1"},   # bins too full: the fallback reads the key range from the header
], ids=lambda e: "-".join(f"{k[5:].lower()}={v}" for k, v in e.items()))
def test_schedules_agree(env, monkeypatch):
    ref = _default(P_WRAP)
    assert ref["num_rendered"] > 0 and any(ref["dL_d" + k].any() for k in NAMES)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _same(ref, _run(_scene(P_WRAP)), str(env))


def test_key_range_across_slots(monkeypatch):
    scene = _scene(P_WRAP, "range")
    z = scene[0][:, 2]
    assert z[0] == z.min() and z[-1] == z.max() and z[-1] / z[0] > 3e4
    ref = _default(P_WRAP, "range")
    assert ref["radii"][0] > 0 and ref["radii"][-1] > 0  # both extremes visible: they set the range
    assert ref["num_rendered"] == _oracle(scene).num_rendered
    monkeypatch.setenv("WGSR_DEPTH_SORT", "global")
    _same(ref, _run(scene), "global vs default")


def test_no_stale_slots():
    before = _run(_scene(65))
    _same(_default(P_WRAP), _run(_scene(P_WRAP)), "large")
    _same(before, _run(_scene(65)), "small after large")
    assert before["num_rendered"] == _oracle(_scene(65)).num_rendered


def test_capacity_mode_counts():
    from wgsr.mapping import rasterize_forward_cap
    ref = _default(P_WRAP)
    N = ref["num_rendered"]
    f = _cam()
    cam = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in f.items()}
    means, opac, scales, rots, shs = (x.to(DEV).contiguous() for x in _scene(P_WRAP))
    counts = torch.zeros(5, dtype=torch.int32, device=DEV)
    out = rasterize_forward_cap(torch.zeros(3, device=DEV), means, opac, scales, rots, shs, 0, cam, H, W, N + 1000,
                                counts)
    c = counts.cpu().tolist()
    assert c[0] == N and c[3] == 0 and 0 < c[2] <= c[1] <= N and c[4] == c[2]
    np.testing.assert_array_equal(out[1].cpu().numpy(), ref["color"])
    np.testing.assert_array_equal(out[2].cpu().numpy(), ref["radii"])
    np.testing.assert_array_equal(out[8].cpu().numpy(), ref["n_touched"])
