"""GPU tests of the fused convex upsampling (csrc/droid_upsample.hip;
wgsr.frontend.cvx_upsample / upsample_disp / upsample / upsample_from_features)
against the float64 oracle tests/_upsample_ref.py and the recorded outputs of
the reference's own code (tests/golden/ref_upsample.npz).

Shapes n x ht x wd: 2 x 3 x 5 (every pixel at a border, wd below the pixel
tile), 1 x 9 x 11 (odd sizes, partial tiles), 3 x 8 x 16 (whole tiles), 1 x 48
x 64 (the tracker's).  Masks are standard normal x 3, rounded to float16 and
also float32; disparities lie in [0.1, 1.1].  ``disps`` / ``disps_up`` are
buffers of n + 3 frames, ``disps_up`` pre-filled with a constant, ``ix`` a
non-monotone selection.  Heads use C = 32, 96 and 128.

Tolerances are derived, never fitted to the kernels (the convention of
tests/test_gpu_reproject.py):

* mask given: the oracle's formula is evaluated once in fp32 numpy; its worst
  error against float64 relative to mag = sum_k w_k |d_k| over the test's own
  outputs is measured, and the GPU is allowed 4 x that (FMA contraction; the
  device's exp and division against numpy's), floor 2^-22, relative to mag.
* the recorded ``FactorGraph.update`` variant (softmax weights rounded to
  float16, which this project never does): the bound above plus 2^-11 mag plus
  9 x 2^-12 max|d| (the rounded weights need not sum to 1).
* head fused in: the kernel's logit (fp32 MFMA sum over C, + bias, one rounding
  to float16) and the exact logit differ by at most delta = 1/2 ulp16 + (C + 2)
  2^-24 (sum |w| |f| + |bias|) (_upsample_ref.logit_delta); logits moved by
  that much move the convex combination by at most (e^{2 delta} - 1) spread / 2
  (_upsample_ref.perturbation_bound, which also shows that the bound holds
  against the oracle's float16-rounded logits); the bound is that per output,
  plus the fp32 bound above.  The same bound holds between the fused call and
  ``upsample`` fed with a torch head's float16 logits (fp32 accumulation, one
  rounding).

Each test prints the worst observed ratio of GPU error to bound.
"""
import os

import numpy as np
import pytest
import torch

import _upsample_ref as ur
from _util import GOLDEN

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22
FILL = -7.0
SHAPES = [(2, 3, 5), (1, 9, 11), (3, 8, 16), (1, 48, 64)]
HEADS = [(2, 3, 5, 32), (1, 9, 11, 96), (3, 8, 16, 128), (3, 8, 16, 32), (1, 48, 64, 128), (1, 48, 64, 96)]
_cache = {}


def _rel_bound(data, mask):
    """(the float64 oracle, the relative fp32 bound) of one input set"""
    r = ur.cvx_upsample(data, mask)
    f = ur.cvx_upsample(data, mask, np.float32)
    assert f["up"].dtype == np.float32
    err = np.abs(f["up"].astype(np.float64) - r["up"])
    assert (r["mag"] > 0).all()
    return r, max(4 * float((err / r["mag"]).max()), FLOOR)


def _case(shape):
    """inputs, oracles and bounds of one shape, computed once and shared (never modified)"""
    if shape in _cache:
        return _cache[shape]
    n, ht, wd = shape
    rng = np.random.default_rng(1000 * n + 10 * ht + wd)
    num = n + 3
    ix = rng.permutation(num)[:n].astype(np.int64)
    if n > 1 and (np.diff(ix) > 0).all():
        ix = ix[::-1].copy()
    disps = rng.uniform(0.1, 1.1, (num, ht, wd)).astype(np.float32)
    masks = {torch.float16: (3 * rng.standard_normal((n, 576, ht, wd))).astype(np.float16),
             torch.float32: (3 * rng.standard_normal((n, 576, ht, wd))).astype(np.float32)}
    c = {"n": n, "ht": ht, "wd": wd, "num": num, "ix": ix, "disps": disps, "masks": masks, "ref": {}, "bound": {}}
    for dt, m in masks.items():
        c["ref"][dt], c["bound"][dt] = _rel_bound(disps[ix][..., None], m)
    c["data4"] = rng.uniform(0.1, 1.1, (n, ht, wd, 4)).astype(np.float32)
    c["dev"] = {"ix": torch.from_numpy(ix).cuda(), "disps": torch.from_numpy(disps).cuda(),
                "masks": {dt: torch.from_numpy(m).cuda() for dt, m in masks.items()},
                "data4": torch.from_numpy(c["data4"]).cuda()}
    _cache[shape] = c
    return c


def _filled(c):
    return torch.full((c["num"], 8 * c["ht"], 8 * c["wd"]), FILL, dtype=torch.float32, device="cuda")


def _check_buffer(c, up, what):
    """frames outside ix hold the constant bit for bit; every addressed element is finite and written"""
    rest = np.setdiff1d(np.arange(c["num"]), c["ix"])
    assert torch.equal(up[torch.from_numpy(rest).cuda()], torch.full_like(up[:len(rest)], FILL)), what
    got = up[c["dev"]["ix"]]
    assert torch.isfinite(got).all() and (got > 0).all(), what
    return got.cpu().numpy().astype(np.float64)[..., None]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["mask16", "mask32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_against_oracle(shape, dtype):
    from wgsr import frontend
    c = _case(shape)
    d = c["dev"]
    up = _filled(c)
    frontend.upsample(d["disps"], up, d["ix"], d["masks"][dtype])
    got = _check_buffer(c, up, "upsample")
    r, b = c["ref"][dtype], c["bound"][dtype]
    ratio = float((np.abs(got - r["up"]) / (b * r["mag"])).max())
    print(f"\nupsample {shape} {dtype}: relative bound {b:.3g}, worst GPU error / bound {ratio:.3f}")
    assert ratio <= 1.0, (ratio, b)
    # the reference's call form: the mask with its leading batch dimension, ix on the host
    up2 = _filled(c)
    frontend.upsample(d["disps"], up2, c["ix"].tolist(), d["masks"][dtype][None])
    assert torch.equal(up, up2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gathered_form_channels_and_repeatability(shape):
    from wgsr import frontend
    c = _case(shape)
    d = c["dev"]
    n, ht, wd = shape
    for dtype in (torch.float16, torch.float32):
        mask = d["masks"][dtype]
        up = _filled(c)
        frontend.upsample(d["disps"], up, d["ix"], mask)
        # src_index / out_index against the gathered form, and the reference's upsample_disp
        gathered = frontend.cvx_upsample(d["disps"][d["ix"]].unsqueeze(-1), mask)
        assert gathered.shape == (n, 8 * ht, 8 * wd, 1) and gathered.dtype == torch.float32
        assert torch.equal(gathered[..., 0], up[d["ix"]])
        disp_up = frontend.upsample_disp(d["disps"][d["ix"]][None], mask[None])
        assert disp_up.shape == (1, n, 8 * ht, 8 * wd) and torch.equal(disp_up[0], gathered[..., 0])
        # dim 2 and 4 agree with dim 1 per channel, bit for bit
        one = [frontend.cvx_upsample(d["data4"][..., k:k + 1].contiguous(), mask)[..., 0] for k in range(4)]
        for dim in (2, 3, 4):
            many = frontend.cvx_upsample(d["data4"][..., :dim].contiguous(), mask)
            assert many.shape == (n, 8 * ht, 8 * wd, dim)
            for k in range(dim):
                assert torch.equal(many[..., k], one[k]), (dtype, dim, k)
        # two runs are bit-identical
        again = _filled(c)
        frontend.upsample(d["disps"], again, d["ix"], mask)
        assert torch.equal(up, again)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_recorded_reference_outputs(tag):
    from wgsr import frontend
    z = np.load(os.path.join(GOLDEN, "ref_upsample.npz"))
    data, mask = z[f"{tag}_data"], z[f"{tag}_mask"]
    dd, dm = torch.from_numpy(data).cuda(), torch.from_numpy(mask).cuda()
    worst = {}
    for dim, name in ((1, "up1"), (2, "up2")):
        r, b = _rel_bound(data[..., :dim], mask)
        rec = z[f"{tag}_{name}"]
        assert np.abs(r["up"] - rec).max() <= 1e-12 * max(1.0, np.abs(rec).max())  # (also tests/test_upsample_ref.py)
        got = frontend.cvx_upsample(dd[..., :dim].contiguous(), dm).cpu().numpy().astype(np.float64)
        worst[name] = float((np.abs(got - rec) / (b * r["mag"])).max())
        if dim == 1:
            disp_up = frontend.upsample_disp(dd[None, ..., 0].contiguous(), dm[None]).cpu().numpy().astype(np.float64)
            worst["disp_up"] = float((np.abs(disp_up - z[f"{tag}_disp_up"]) / (b * r["mag"][None, ..., 0])).max())
            # the update path of the reference rounds its softmax weights to float16
            upd = z[f"{tag}_up1_update"].astype(np.float64)
            bound = b * r["mag"] + 2.0 ** -11 * r["mag"] + 9 * 2.0 ** -12 * np.abs(data[..., :1]).max()
            worst["update"] = float((np.abs(got - upd) / bound).max())
    print(f"\nfixture {tag}: worst GPU error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def _head_case(n, ht, wd, C):
    key = (n, ht, wd, C)
    if key in _cache:
        return _cache[key]
    c = _case((n, ht, wd))
    rng = np.random.default_rng(7 * C + ht)
    feat = rng.standard_normal((n, C, ht, wd)).astype(np.float16)
    weight = (3.0 / np.sqrt(C) * rng.standard_normal((576, C))).astype(np.float16)
    bias = (0.5 * rng.standard_normal(576)).astype(np.float32)
    h = ur.head(feat, weight, bias)
    r, b = _rel_bound(c["disps"][c["ix"]][..., None], h["logits"])
    bound = ur.perturbation_bound(ur.logit_delta(h, C), r["spread"]) + b * r["mag"]
    _cache[key] = (feat, weight, bias, r, bound)
    return _cache[key]


@pytest.mark.parametrize("n,ht,wd,C", HEADS)
def test_upsample_from_features(n, ht, wd, C):
    from wgsr import frontend
    c = _case((n, ht, wd))
    d = c["dev"]
    feat, weight, bias, r, bound = _head_case(n, ht, wd, C)
    df, dw, db = (torch.from_numpy(a).cuda() for a in (feat, weight, bias))
    up = _filled(c)
    frontend.upsample_from_features(d["disps"], up, d["ix"], df, dw, db)
    got = _check_buffer(c, up, "upsample_from_features")
    ratio = float((np.abs(got - r["up"]) / bound).max())
    # against upsample fed with a torch head's float16 logits (fp32 accumulation, one rounding)
    logits = (torch.matmul(dw.float(), df.float().view(n, C, ht * wd)) + db[:, None]).half().view(n, 576, ht, wd)
    via = _filled(c)
    frontend.upsample(d["disps"], via, d["ix"], logits)
    ratio_torch = float((np.abs(got - _check_buffer(c, via, "upsample")) / bound).max())
    share = float((logits.cpu().numpy().astype(np.float64) == ur.head(feat, weight, bias)["logits"]).mean())
    print(f"\nfused head {n}x{ht}x{wd} C={C}: worst GPU error / bound: oracle {ratio:.3f}, torch head {ratio_torch:.3f}"
          f" (torch logits equal to the oracle's: {share:.4f})")
    assert ratio <= 1.0 and ratio_torch <= 1.0, (ratio, ratio_torch)
    # the Conv2d's own parameters: [576, C, 1, 1] float32 weight (float16 values), converted once and cached
    up2 = _filled(c)
    w4 = dw.float().view(576, C, 1, 1)
    frontend.upsample_from_features(d["disps"], up2, d["ix"], df[None], w4, db)
    assert torch.equal(up, up2)
    again = _filled(c)
    frontend.upsample_from_features(d["disps"], again, d["ix"], df, w4, db)
    assert torch.equal(up, again)


def test_fused_head_with_every_cu_busy():
    """24 frames of 48 x 64 (2304 workgroups, several resident per CU): a
    development build whose accumulators the compiler split over two register
    files was right at every smaller size and wrong in a few 16-pixel groups
    here, in about every second run.  Checked on the device alone: where the
    kernel's nine logits equal a torch head's (fp32 accumulation, one rounding)
    the two kernels share every later instruction, so the outputs are bit-equal;
    elsewhere (one of an output's nine logits on a rounding boundary, each in
    about 1 of 1000: a share well under 5 % of the outputs) the logits are at
    most one float16 ulp apart and the outputs at most (e^{2 u} - 1) / 2 x the
    largest disparity, u = ulp16(max |logit|)."""
    from wgsr import frontend
    n, ht, wd, C = 24, 48, 64, 128
    g = torch.Generator(device="cuda").manual_seed(24)
    disps = 0.1 + torch.rand(2 * n, ht, wd, device="cuda", generator=g)
    ix = torch.randperm(2 * n, device="cuda", generator=g)[:n].contiguous()
    feat = torch.randn(n, C, ht, wd, device="cuda", generator=g).half()
    weight = (3.0 / C ** 0.5 * torch.randn(576, C, device="cuda", generator=g)).half()
    bias = 0.5 * torch.randn(576, device="cuda", generator=g)
    logits = (torch.matmul(weight.float(), feat.float().view(n, C, ht * wd)) + bias[:, None]).half().view(n, 576, ht, wd)
    ref = torch.full((2 * n, 8 * ht, 8 * wd), FILL, device="cuda")
    frontend.upsample(disps, ref, ix, logits)
    u = float(ur.ulp_fp16(float(logits.abs().max())))
    bound = float(np.expm1(2 * u)) / 2 * float(disps.max())
    for rep in range(4):
        up = torch.full_like(ref, FILL)
        frontend.upsample_from_features(disps, up, ix, feat, weight, bias)
        differ = up != ref
        share, worst = float(differ.float().mean()), float((up - ref).abs().max())
        print(f"\nrun {rep}: outputs that differ {share:.5f}, largest difference {worst:.3g} (bound {bound:.3g})")
        assert share < 0.05 and worst <= bound, (rep, share, worst, bound)


def test_head_parameter_cache_follows_the_parameter():
    from wgsr import frontend
    n, ht, wd, C = HEADS[0]
    c = _case((n, ht, wd))
    d = c["dev"]
    feat, weight, bias, _, _ = _head_case(n, ht, wd, C)
    df, db = torch.from_numpy(feat).cuda(), torch.from_numpy(bias).cuda()
    w = torch.from_numpy(weight).cuda().float().view(576, C, 1, 1)
    a, b, e = _filled(c), _filled(c), _filled(c)
    frontend.upsample_from_features(d["disps"], a, d["ix"], df, w, db)
    w.mul_(-1.0)  # the same storage, a new version: the float16 copy must be remade
    frontend.upsample_from_features(d["disps"], b, d["ix"], df, w, db)
    frontend.upsample_from_features(d["disps"], e, d["ix"], df, w.half().view(576, C), db)
    assert torch.equal(b, e) and not torch.equal(a, b)
    # another tensor at a freed tensor's address (same shape, version 0 again) is not served the old copy
    for scale in (1.0, 2.0, 3.0):
        tmp = (scale * torch.from_numpy(weight).cuda()).float().view(576, C, 1, 1)
        got, want = _filled(c), _filled(c)
        frontend.upsample_from_features(d["disps"], got, d["ix"], df, tmp, db)
        frontend.upsample_from_features(d["disps"], want, d["ix"], df, tmp.half().view(576, C), db)
        assert torch.equal(got, want), scale
        del tmp


def test_out_of_range_index_raises_and_writes_nothing():
    from wgsr import frontend
    c = _case(SHAPES[2])
    d = c["dev"]
    feat, weight, bias, _, _ = _head_case(*SHAPES[2], 128)
    df, dw, db = (torch.from_numpy(a).cuda() for a in (feat, weight, bias))
    for bad_value in (c["num"], -1):
        bad = d["ix"].clone()
        bad[1] = bad_value
        up = _filled(c)
        with pytest.raises(RuntimeError, match="outside"):
            frontend.upsample(d["disps"], up, bad, d["masks"][torch.float16])
        assert torch.equal(up, _filled(c))
        with pytest.raises(RuntimeError, match="outside"):
            frontend.upsample_from_features(d["disps"], up, bad, df, dw, db)
        assert torch.equal(up, _filled(c))
        # unchecked: no exception, and still nothing written
        frontend.upsample(d["disps"], up, bad, d["masks"][torch.float16], check=False)
        frontend.upsample_from_features(d["disps"], up, bad, df, dw, db, check=False)
        torch.cuda.synchronize()
        assert torch.equal(up, _filled(c))
    # the two buffers may differ in length: the range of each is its own
    short = torch.full((3, 64, 128), FILL, device="cuda")
    with pytest.raises(RuntimeError, match="output frames"):
        frontend.upsample(d["disps"], short, torch.tensor([0, 1, 3], device="cuda"), d["masks"][torch.float16])
    assert torch.equal(short, torch.full_like(short, FILL))


def test_argument_errors():
    from wgsr import frontend
    c = _case(SHAPES[0])
    d = c["dev"]
    n, ht, wd = SHAPES[0]
    mask = d["masks"][torch.float16]
    up = _filled(c)
    feat = torch.zeros(n, 32, ht, wd, dtype=torch.float16, device="cuda")
    w, b = torch.zeros(576, 32, dtype=torch.float16, device="cuda"), torch.zeros(576, device="cuda")
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.cvx_upsample(d["data4"].cpu(), mask.cpu())
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.upsample(d["disps"].cpu(), up, d["ix"], mask)
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.upsample(d["disps"], up, d["ix"], mask.cpu())
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.upsample_from_features(d["disps"], up, d["ix"], feat.cpu(), w, b)
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="mask requires grad"):
            frontend.upsample(d["disps"], up, d["ix"], mask.clone().requires_grad_())
        with pytest.raises(NotImplementedError, match="data requires grad"):
            frontend.cvx_upsample(d["data4"].clone().requires_grad_(), mask)
        with pytest.raises(NotImplementedError, match="weight requires grad"):
            frontend.upsample_from_features(d["disps"], up, d["ix"], feat, w.clone().requires_grad_(), b)
    with torch.no_grad():  # inference: a parameter that requires grad is fine when grad mode is off
        frontend.upsample_from_features(d["disps"], up, d["ix"], feat, w.clone().requires_grad_(), b)
    with pytest.raises(ValueError, match="mask"):
        frontend.upsample(d["disps"], up, d["ix"], mask[:, :575].contiguous())
    with pytest.raises(ValueError, match="mask"):
        frontend.cvx_upsample(d["data4"][..., :1].contiguous(), mask[:, :64].contiguous())
    with pytest.raises(NotImplementedError, match="dim"):
        frontend.cvx_upsample(torch.zeros(n, ht, wd, 5, device="cuda"), mask)
    with pytest.raises(NotImplementedError, match="feat"):
        frontend.upsample_from_features(d["disps"], up, d["ix"], feat.float(), w, b)
    with pytest.raises(ValueError, match="C = 48"):
        frontend.upsample_from_features(d["disps"], up, d["ix"], feat.repeat(1, 2, 1, 1)[:, :48].contiguous(),
                                        torch.zeros(576, 48, dtype=torch.float16, device="cuda"), b)
    with pytest.raises(ValueError, match="weight"):
        frontend.upsample_from_features(d["disps"], up, d["ix"], feat, w[:500].contiguous(), b)
    with pytest.raises(ValueError, match="disps_up"):
        frontend.upsample(d["disps"], up[:, :-8].contiguous(), d["ix"], mask)
    torch.cuda.synchronize()
    assert torch.equal(up[np.setdiff1d(np.arange(c["num"]), c["ix"])], _filled(c)[:3])
    # no entries: nothing to do
    frontend.upsample(d["disps"], up, d["ix"][:0], mask[:0])
    assert frontend.cvx_upsample(d["data4"][:0], mask[:0]).shape == (0, 8 * ht, 8 * wd, 4)


def test_single_frame_and_unchecked_graph_capture():
    """len(ix) == 1 (the reference's .squeeze() case), and check=False makes no
    host read: the call is captured (one branch) and replays to the same bits"""
    from wgsr import frontend
    c = _case(SHAPES[2])
    d = c["dev"]
    mask = d["masks"][torch.float16]
    full = _filled(c)
    frontend.upsample(d["disps"], full, d["ix"], mask)
    one = _filled(c)
    frontend.upsample(d["disps"], one, d["ix"][1:2], mask[1:2])
    k = int(c["ix"][1])
    assert torch.equal(one[k], full[k])
    one[k] = FILL
    assert torch.equal(one, _filled(c))

    feat, weight, bias, _, _ = _head_case(*SHAPES[2], 128)
    df, dw, db = (torch.from_numpy(a).cuda() for a in (feat, weight, bias))
    fused = _filled(c)
    frontend.upsample_from_features(d["disps"], fused, d["ix"], df, dw, db)
    torch.cuda.synchronize()
    a, b = _filled(c), _filled(c)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frontend.upsample(d["disps"], a, d["ix"], mask, check=False)
        frontend.upsample_from_features(d["disps"], b, d["ix"], df, dw, db, check=False)
    a.fill_(FILL)
    b.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, full) and torch.equal(b, fused)
