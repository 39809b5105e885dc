"""GPU: csrc/mapping.hip element by element against the float64 oracle, through
its C ABI on the test's own inputs, with no rasteriser behind it
(tests/_map_elementwise_ref.py holds the cases, the decisions and the bound;
tests/test_map_elementwise_ref.py shows on the CPU that the check fails on an
isotropic term without its - sm and on a normalise backward without its
projection term).

* wgsr_gaussian_activate: opacity, scales, rotations per element, every
  workgroup's isotropic partial sum and their sum; raw opacities of +-20, raw
  scales from -9 to 3, a quaternion of norm 1e-20 and an all-zero one.
* wgsr_gaussian_activate_backward: the three raw gradients per element
  against float64 autograd, iso_weight 0 and 10 / 3P; rows with three and
  with two bit-equal scales, the rows under the quaternion floor.
* ..._backward_stats and wgsr_densification_stats: max_radii2D and denom
  exact, grad_accum inside the bound, rows with radii <= 0 and every row under
  a set skip word keep their bits, the two entries agree bit for bit.
* wgsr_mapping_loss_forward / _backward: image_ab, d_image, d_depth per pixel,
  every workgroup's partials and their sums, with and without an SSIM plane.

Every output buffer is guarded: the guard stays untouched and every output
element is written.  P = 1, 255, 257, 1000; images 1x1, 7x37, 16x16, 33x129.
"""
import numpy as np
import pytest
import torch

import _map_elementwise_ref as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lib():
    from wgsr import _lib as lib
    return lib, lib.load()


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("P", E.MAP_P)
def test_activate_elements_match_the_float64_oracle(P):
    lib, L = _lib()
    c = E.act_case(P, 0.0)
    nb = int(L.wgsr_map_blocks(P))
    assert nb == (P + E.WGROUP - 1) // E.WGROUP
    o, s, q = (_d(c.inp[k]) for k in ("o", "s", "q"))
    op, sc, rot, iso = E.Guarded((P,)), E.Guarded((P, 3)), E.Guarded((P, 4)), E.Guarded((nb,))
    with torch.cuda.device(DEV):
        lib.check(L.wgsr_gaussian_activate(P, lib.ptr(o), lib.ptr(s), lib.ptr(q), op.ptr(), sc.ptr(), rot.ptr(),
                                           iso.ptr(), lib.stream_handle(DEV)))
    torch.cuda.synchronize()
    got = dict(opacity=op.read(), scales=sc.read(), rotations=rot.read(), iso_part=iso.read())
    E.act_check_forward(c, got)
    if P > 16:   # the zero quaternion stays a zero row
        assert not got["rotations"][10].any()


def _backward(c, stats=None, skip=None, entry="plain"):
    """-> (raw gradients, statistics after the call)."""
    lib, L = _lib()
    P = c.P
    ins = [_d(c.inp[k]) for k in ("o", "s", "q", "g_op", "g_sc", "g_rot")]
    d_o, d_s, d_r = E.Guarded((P,)), E.Guarded((P, 3)), E.Guarded((P, 4))
    st = {k: E.Guarded((P,), init=c.inp[k]) for k in ("max_radii", "accum", "denom")}
    radii, m2d = _d(c.inp["radii"]), _d(c.inp["m2d"])
    stream = lib.stream_handle(DEV)
    with torch.cuda.device(DEV):
        if entry == "plain":
            lib.check(L.wgsr_gaussian_activate_backward(P, *[lib.ptr(t) for t in ins], c.iso_w, d_o.ptr(), d_s.ptr(),
                                                        d_r.ptr(), stream))
        elif entry == "stats":
            word = None if skip is None else _d(np.array([skip], np.uint32).view(np.int32))
            lib.check(L.wgsr_gaussian_activate_backward_stats(
                P, *[lib.ptr(t) for t in ins], c.iso_w, d_o.ptr(), d_s.ptr(), d_r.ptr(), lib.ptr(radii), lib.ptr(m2d),
                st["max_radii"].ptr(), st["accum"].ptr(), st["denom"].ptr(), lib.ptr(word), stream))
        else:
            lib.check(L.wgsr_densification_stats(P, lib.ptr(radii), lib.ptr(m2d), st["max_radii"].ptr(),
                                                 st["accum"].ptr(), st["denom"].ptr(), stream))
    torch.cuda.synchronize()
    grads = None if entry == "densify" else dict(d_o=d_o.read(), d_s=d_s.read(), d_r=d_r.read())
    return grads, {k: v.read(written=False) for k, v in st.items()}


@pytest.mark.parametrize("P", E.MAP_P)
@pytest.mark.parametrize("iso", E.ISO_WEIGHTS)
def test_activate_backward_elements_match_float64_autograd(P, iso):
    c = E.act_case(P, iso)
    got, stats = _backward(c)
    E.act_check_backward(c, got)
    for k in stats:   # the plain entry has no statistics to touch
        assert np.array_equal(_bits(stats[k]), _bits(c.inp[k]))


@pytest.mark.parametrize("P", E.MAP_P)
def test_densification_statistics(P):
    c = E.act_case(P, "10/3P")
    plain, _ = _backward(c)
    fused, st = _backward(c, entry="stats")
    _, st2 = _backward(c, entry="densify")
    _, st0 = _backward(c, entry="stats", skip=0)
    skipped, st_skip = _backward(c, entry="stats", skip=1)
    for k in ("d_o", "d_s", "d_r"):   # the raw gradients are written whatever the statistics do
        assert np.array_equal(_bits(fused[k]), _bits(plain[k])), k
        assert np.array_equal(_bits(skipped[k]), _bits(plain[k])), k
    assert np.array_equal(st["max_radii"], c.stats["max_radii"]) and np.array_equal(st["denom"], c.stats["denom"])
    rep = E.Report(f"densify P{P}")
    E._check(rep, "densify", "grad_accum", st["accum"], c.o64["accum"], c.o32["accum"])
    rep.finish()
    for k in st:
        assert np.array_equal(_bits(st[k][~c.vis]), _bits(c.inp[k][~c.vis])), f"{k}: a row with radii <= 0 changed"
        assert np.array_equal(_bits(st2[k]), _bits(st[k])), f"{k}: the two entries differ"
        assert np.array_equal(_bits(st0[k]), _bits(st[k])), f"{k}: a clear skip word changed the statistics"
        assert np.array_equal(_bits(st_skip[k]), _bits(c.inp[k])), f"{k}: written under a set skip word"


@pytest.mark.parametrize("H,W", E.MAP_IMAGES)
@pytest.mark.parametrize("use_ssim", [False, True])
def test_mapping_loss_pixels_match_the_float64_oracle(H, W, use_ssim):
    lib, L = _lib()
    c = E.maploss_case(H, W, use_ssim)
    nb = int(L.wgsr_map_blocks(H * W))
    t = {k: v.to(DEV).contiguous() for k, v in c.t.items()}
    image_ab, part = E.Guarded((3, H, W)), E.Guarded((nb, 2))
    d_image, d_depth, part_b = E.Guarded((3, H, W)), E.Guarded((1, H, W)), E.Guarded((nb, 2))
    p, stream = lib.ptr, lib.stream_handle(DEV)
    with torch.cuda.device(DEV):
        lib.check(L.wgsr_mapping_loss_forward(H, W, p(t["ren"]), p(t["gt"]), p(t["dep"]), p(t["gd"]), p(t["ea"]),
                                              p(t["eb"]), E.RGB_TH, image_ab.ptr(), part.ptr(), stream))
        lib.check(L.wgsr_mapping_loss_backward(H, W, p(t["ren"]), image_ab.ptr(), p(t["gt"]), p(t["dep"]), p(t["gd"]),
                                               p(t["ea"]), E.RGB_TH, E.MAPLOSS_W[0], E.MAPLOSS_W[1],
                                               p(t["ssim"]) if use_ssim else None, d_image.ptr(), d_depth.ptr(),
                                               part_b.ptr(), stream))
    torch.cuda.synchronize()
    fw, bw = part.read(), part_b.read()
    E.maploss_check(c, dict(image_ab=image_ab.read(), d_image=d_image.read(), d_depth=d_depth.read(),
                            part_l1=fw[:, 0], part_l1d=fw[:, 1], part_da=bw[:, 0], part_db=bw[:, 1]))
