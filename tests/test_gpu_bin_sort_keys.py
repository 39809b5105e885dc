"""The bin sort's wide pass at every workgroup size (WGSR_BIN_SORT_THREADS):
256, 512 or 1024 threads rank the same tile of keys, so the sorted pairs --
and with them every list -- must not change.  The default build is compared
bit for bit (images, radii, n_touched, num_rendered, every gradient) with
  WGSR_BIN_SORT_THREADS=256/512/1024   each workgroup size of the wide pass,
  WGSR_BIN_SHIFT=0 WGSR_DEPTH_SORT=bins  the exact per-tile pairs: the same
                                       lists built without the bin sort,
and one case per shape family with the CPU restatement (tolerances of
test_gpu_raster).  (The depth keys that the sort's last pass was to write
beside the ids, and their WGSR_BDS_KEYS switch, were measured slower and are
not in the library -- DESIGN.md section 8 -- so there is nothing of them to
compare; the shapes chosen for them stay, as every one is also a shape of the
sort or of the lists behind it.)

Shapes: the smallest at which each path can go wrong.
  wide9    544x512, 2x2-tile bins: 17 x 16 = 272 bins, 9 key bits, the <512>
           wide pass; 30 000 Gaussians give several tiles of pairs with a
           partial last one.
  wide10   1056x512: 33 x 16 = 528 bins, 10 bits, the <1024> wide pass.
  few      wide9's frame with 1 500 Gaussians: fewer pairs than one tile (one
           partial workgroup, most digits empty).
  ragged   100x72 at 4x4- and 2x2-tile bins, and
  small    200x136 (default opacities): test_gpu_bin_emit's shapes -- at most
           256 bins, the single 8-bit scatter; bins under 64 entries and
           empty bins.
  big_bin  64x64, 20 000 Gaussians, one bin beyond three LDS tiles.
  two_pass 1056x1024: 33 x 32 = 1056 bins, 11 bits, a two-pass bin sort (no
           wide pass: the setting must be ignored).
The opacity-0.05 scenes reach most of their bins (no pixel terminates early):
test_scenes_reach_their_bins checks on the CPU restatement that more than
half of each frame's bins hold a covered pixel and that the Gaussians with
n_touched > 0 outnumber the bins.

The CPU restatement is compared on the wide frames with the scene's own
opacities (wide9_own, wide10_own, two_pass_own), not at opacity 0.05: there
the first contributor of a pixel sits at transmittance ~1, so one alpha =
1/255 threshold flip (__expf against expf) moves the depth image by up to
depth / 255 = 0.0157 at depth 4, above check_against's bound of 0.01 x the
image's largest value (1.4 at that opacity).  The parent library differs
from the restatement by exactly that on wide9 (0.015666 in one pixel); the
bound is test_gpu_raster's and stays.

WGSR_BIN_DEPTH_MAX_AVG is raised for every run and every run with sort bins
asserts that the per-bin schedule ran (wgsr_depth_order_offset() == -1).
"""
import numpy as np
import pytest
import torch

from test_gpu_raster import _cpu_expect, _synthetic, check_against, run_c

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (W, H, P, SH degree, every opacity or None for the scene's own, bin shift)
SHAPES = {
    "wide9": (544, 512, 30_000, 0, 0.05, 1),
    "wide10": (1056, 512, 30_000, 0, 0.05, 1),
    "few": (544, 512, 1_500, 0, 0.05, 1),
    "ragged_s2": (100, 72, 30_000, 1, 0.05, 2),
    "ragged_s1": (100, 72, 30_000, 1, 0.05, 1),
    "small": (200, 136, 6_000, 1, None, 1),
    "big_bin": (64, 64, 20_000, 0, 0.05, 2),
    "two_pass": (1056, 1024, 30_000, 0, 0.05, 1),
    "wide9_own": (544, 512, 30_000, 0, None, 1),
    "wide10_own": (1056, 512, 30_000, 0, None, 1),
    "two_pass_own": (1056, 1024, 30_000, 0, None, 1),
}
CPU_CHECKED = ("wide9_own", "wide10_own", "small", "big_bin", "two_pass_own")  # one per family
VARIANTS = (("WGSR_BIN_SORT_THREADS", "256"), ("WGSR_BIN_SORT_THREADS", "512"), ("WGSR_BIN_SORT_THREADS", "1024"))
_ENV = ("WGSR_BIN_SORT_THREADS", "WGSR_DEPTH_SORT")
_cache = {}


def _bins(shape):
    W, H, _, _, _, shift = SHAPES[shape]
    b = 16 << shift
    return (W + b - 1) // b, (H + b - 1) // b


def _inputs(shape):
    key = ("in",) + SHAPES[shape][:5]
    if key not in _cache:
        W, H, P, deg, opac, _ = SHAPES[shape]
        inputs, settings, grads = _synthetic(P, W, H, deg)
        if opac is not None:
            inputs = dict(inputs, opacities=torch.full_like(inputs["opacities"], opac))
        _cache[key] = (inputs, settings, grads)
    return _cache[key]


def _cpu(shape):
    key = ("cpu",) + SHAPES[shape][:5]
    if key not in _cache:
        _cache[key] = _cpu_expect(*_inputs(shape))
    return _cache[key]


def _depth_order_offset():
    from wgsr import _lib
    return int(_lib.load().wgsr_depth_order_offset())


def _setenv(monkeypatch, shift, env=()):
    monkeypatch.setenv("WGSR_BIN_DEPTH_MAX_AVG", "100000000")
    monkeypatch.setenv("WGSR_BIN_SHIFT", str(shift))
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)


def _run(shape, monkeypatch, shift, env=()):
    _setenv(monkeypatch, shift, env)
    offs = []
    out = run_c(*_inputs(shape), between=lambda: offs.append(_depth_order_offset()))
    # (without sort bins there is no per-bin sort: the exact pairs follow a Gaussian-level depth order)
    assert shift == 0 or offs[0] == -1, "the per-bin depth sort did not run"
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k, v in a.items():
        if k == "num_rendered":
            assert b[k] == v, what
        else:
            np.testing.assert_array_equal(b[k], v, err_msg=f"{what}: {k}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_workgroup_sizes_change_nothing(shape, monkeypatch):
    shift = SHAPES[shape][5]
    out = _run(shape, monkeypatch, shift)
    assert out["num_rendered"] > 0
    for env in VARIANTS:
        _same(out, _run(shape, monkeypatch, shift, (env,)), f"{shape} vs {env[0]}={env[1]}")
    # the exact per-tile pairs, each tile's by depth: the same lists without the bin sort
    _same(out, _run(shape, monkeypatch, 0, (("WGSR_DEPTH_SORT", "bins"),)), f"{shape} vs exact per-tile lists")
    if shape in CPU_CHECKED:
        check_against(out, _cpu(shape))


def test_full_size_tiles(monkeypatch):
    """1M Gaussians at 1080p, the frame's own 4x4-tile bins: more than 2M
    pairs, so the sort works on 4096-key tiles -- the only size at which the
    256- and 512-thread workgroups find their peer groups through the LDS
    lane-mask table; at 1024 threads the table does not fit and the ballots
    do it.  All three must sort alike.  (test_gpu_raster's 1M case compares
    this frame with the CPU restatement.)"""
    inputs, settings, grads = _synthetic(1_000_000, 1920, 1080, 0)
    outs = []
    for threads in (None, "256", "1024"):
        _setenv(monkeypatch, 2, (("WGSR_BIN_SORT_THREADS", threads),) if threads else ())
        outs.append(run_c(inputs, settings, grads, between=lambda: outs.append(_depth_order_offset())))
    assert outs[0] == outs[2] == outs[4] == -1, "the per-bin depth sort did not run"
    assert outs[1]["num_rendered"] > (1 << 21)
    _same(outs[1], outs[3], "512 vs 256 threads")
    _same(outs[1], outs[5], "512 vs 1024 threads")


@pytest.mark.parametrize("shape", [s for s in SHAPES if SHAPES[s][4] is not None and s != "few"])
def test_scenes_reach_their_bins(shape):
    """The constants above, on the CPU restatement: more than half of the
    frame's bins hold a covered pixel (so at least one Gaussian), and the
    Gaussians that reach a list outnumber the bins."""
    W, H, _, _, _, shift = SHAPES[shape]
    bx, by = _bins(shape)
    exp = _cpu(shape)
    b = 16 << shift
    cov = np.zeros((by * b, bx * b), bool)
    cov[:H, :W] = exp["opacity"].reshape(H, W) > 0
    occupied = int(cov.reshape(by, b, bx, b).any(axis=(1, 3)).sum())
    assert 2 * occupied > bx * by, (occupied, bx * by)
    assert int(np.count_nonzero(exp["n_touched"] > 0)) > bx * by


def test_all_culled(monkeypatch):
    """Every mean behind the camera on the wide pass's frame: no pair, no
    sort -- no error, and the images are the background."""
    from diff_gaussian_rasterization import _C
    from wgsr.camera import synthetic_camera
    W, H, P = 544, 512, 1_500
    _setenv(monkeypatch, 1)
    f = synthetic_camera(W, H, 0).raster_fields()
    e = torch.empty(0, device=DEV)
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    bg = torch.tensor([0.25, 0.5, 0.75], device=DEV)
    m = z(P, 3)
    m[:, 2] = -1.0
    q = z(P, 4)
    q[:, 0] = 1
    out = _C.rasterize_gaussians(bg, m, e, z(P, 1) + 0.5, z(P, 3) + 0.01, q, 1.0, e, f["viewmatrix"].to(DEV),
                                 f["projmatrix"].to(DEV), f["projmatrix_raw"].to(DEV), f["tanfovx"], f["tanfovy"],
                                 H, W, z(P, 1, 3), 0, f["campos"].to(DEV), False, False)
    nr, color, radii, _, _, _, depth, opac, _ = out
    torch.cuda.synchronize()
    assert nr == 0 and int(radii.abs().sum()) == 0
    np.testing.assert_array_equal(color.cpu().numpy(),
                                  np.broadcast_to(bg.cpu().numpy()[:, None, None], (3, H, W)))
    assert float(opac.abs().sum()) == 0.0 and float(depth.abs().sum()) == 0.0


@pytest.mark.parametrize("threads", [None, "1024"])
def test_capacity_forward(threads, monkeypatch):
    """Capacity mode on the 200x136 scene, called as test_gpu_online_graph
    calls it, at capacities N_rect + 1 and 4 N_rect (most pair slots of the
    larger one are never written: nothing may be read through them).  Outputs
    and gradients equal the host-synchronised forward's."""
    from diff_gaussian_rasterization import _C
    from wgsr.mapping import check_tile_lists, rasterize_forward_cap
    W, H, _, deg, _, shift = SHAPES["small"]
    inputs, st, grads = _inputs("small")
    _setenv(monkeypatch, shift, (("WGSR_BIN_SORT_THREADS", threads),) if threads else ())
    d = lambda x: x.to(DEV).contiguous()  # noqa: E731
    e = torch.empty(0, device=DEV)
    bg, xyz, opac, scales, rots, shs = (d(st["bg"]), d(inputs["means3D"]), d(inputs["opacities"]),
                                        d(inputs["scales"]), d(inputs["rotations"]), d(inputs["shs"]))
    cam = {k: (d(st[k]) if torch.is_tensor(st[k]) else st[k])
           for k in ("viewmatrix", "projmatrix", "projmatrix_raw", "campos", "tanfovx", "tanfovy")}
    dcol, ddep = d(grads[0]), d(grads[1])

    def backward(fwd):
        return _C.rasterize_gaussians_backward(bg, xyz, fwd[2], e, scales, rots, 1.0, e, cam["viewmatrix"],
                                               cam["projmatrix"], cam["projmatrix_raw"], cam["tanfovx"],
                                               cam["tanfovy"], dcol, ddep, shs, deg, cam["campos"], fwd[3], fwd[0],
                                               fwd[4], fwd[5], False)

    ref = _C.rasterize_gaussians(bg, xyz, e, opac, scales, rots, 1.0, e, cam["viewmatrix"], cam["projmatrix"],
                                 cam["projmatrix_raw"], cam["tanfovx"], cam["tanfovy"], H, W, shs, deg, cam["campos"],
                                 False, False)
    assert _depth_order_offset() == -1
    N = ref[0]
    assert N > 1000
    gr = backward(ref)
    counts = torch.zeros(5, dtype=torch.int32, device=DEV)
    bad = torch.zeros(3, dtype=torch.int32, device=DEV)
    for cap in (N + 1, 4 * N):
        counts.zero_()
        out = rasterize_forward_cap(bg, xyz, opac, scales, rots, shs, deg, cam, H, W, cap, counts)
        assert _depth_order_offset() == -1
        c = counts.cpu().tolist()
        assert c[0] == N and c[3] == 0 and 0 < c[2] <= c[1] <= N and c[4] == c[2]
        for i in (1, 2, 6, 7, 8):
            assert torch.equal(out[i], ref[i]), (cap, i)
        check_tile_lists(out, xyz, cam, H, W, deg, shs, bad)
        assert bad.tolist() == [0, 0, 0]
        for a, b in zip(gr, backward(out)):
            assert torch.equal(a, b), cap
