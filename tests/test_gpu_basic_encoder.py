"""GPU tests of the tracker's feature and context encoders
(csrc/droid_basic_encoder.hip; wgsr.frontend.feature_encoder / context_encoder)
against the float64 oracle tests/_basic_encoder_ref.py and the recorded outputs
of the reference's own BasicEncoder (tests/golden/ref_basic_encoder.npz).

Shapes n x H x W, for both encoders: 2 x 16 x 24 (every map smaller than one
tile, the last map 2 x 3), 1 x 37 x 53 (odd at every level -- 19 x 27, 10 x 14,
5 x 7: ceil sizes, the stride-2 tap past the last row and column, partial tiles
in the statistics), 3 x 64 x 128 (whole tiles at every level), 1 x 72 x 136
(several tiles and partial ones).

1. Per launch, teacher-forced: the GPU's own stored inputs of launch k go to the
   oracle's launch k, and every element of every raw map, side output and
   statistic lies within the oracle's derived bound d (nothing fitted; depth
   does not loosen it).
2. End to end against the plain float64 evaluation (and, at the fixture's cases,
   the recorded reference): with E16 = rms(oracle with the contract's rounding
   points - plain oracle), rms(GPU - plain) <= 2 E16.  Two evaluations with the
   same rounding points and different arithmetic differ from each other by
   about E16, so sqrt(2) E16 is expected and 2 leaves room.
3. Structural, exact: frames of a batch, runs, call forms; the receptive field;
   zero padding after the transformation; mean / std; one-hot taps.
4. Graph capture.  5. Argument errors.

Every result buffer is a guarded one (FILL / GUARD).
"""
import numpy as np
import pytest
import torch

import _basic_encoder_ref as br

pytestmark = pytest.mark.gpu

FILL = -60000.0      # (float16 holds it; no map of these tests comes near it)
GUARD = 64
SHAPES = br.GPU_SHAPES
NORMS = ("instance", "none")
_cache = {}


def _ids(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


def _state_dict(P, prefix=""):
    sd = {}
    for name, (w, b) in P.items():
        sd[f"{prefix}{name}.weight"] = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        sd[f"{prefix}{name}.bias"] = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    return sd


def _guarded(shape, dtype=torch.float16):
    whole = torch.full((int(np.prod(shape)) + GUARD,), FILL, dtype=dtype, device="cuda")
    return whole, whole[:-GUARD].view(shape)


def _run(norm, images, params, **kw):
    """the encoder into guarded buffers -> its outputs on the device (a tuple) and what the call returned besides"""
    from wgsr import frontend
    x = images[0] if images.dim() == 5 else images
    shape = (x.shape[0], 128) + frontend.be_sizes(x.shape[2], x.shape[3])[2]
    bufs = [_guarded(shape) for _ in range(1 if norm == "instance" else 2)]
    outs = tuple(b[1] for b in bufs)
    f = frontend.feature_encoder if norm == "instance" else frontend.context_encoder
    got = f(images, params, out=outs[0] if norm == "instance" else outs, **kw)
    extra = None
    if kw.get("return_intermediates"):
        got, extra = got
    got = (got,) if norm == "instance" else tuple(got)
    for g, (whole, out) in zip(got, bufs):
        assert g is out and bool((whole[-GUARD:] == FILL).all())
    if shape[0]:
        assert not any(bool((o == FILL).any()) for o in outs)       # every element is written
    return outs, extra


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _case(norm, shape):
    """the shared oracle case (tests/_basic_encoder_ref.shape_case) with the GPU's results, computed once"""
    key = (norm, shape)
    if key not in _cache:
        from wgsr import frontend
        c = dict(br.shape_case(norm, shape))
        c["sd"] = _state_dict(c["P"], "fnet." if norm == "instance" else "cnet.")
        c["params"] = frontend.BasicEncoder.from_state_dict(c["sd"], "fnet." if norm == "instance" else "cnet.", norm)
        c["dev"] = torch.from_numpy(c["images"]).cuda()
        c["gpu"], inter = _run(norm, c["dev"], c["params"], return_intermediates=True)
        c["inter"] = {k: v.clone() for k, v in inter.items()}
        _cache[key] = c
    return _cache[key]


def _outputs(norm, ev):
    return (ev["out"],) if norm == "instance" else (ev["net"], ev["inp"])


def _within(got, ref, d, worst, name):
    """|got - ref| <= d everywhere (d may be zero: then the bits agree); the worst ratio goes into ``worst``"""
    got = _np(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), name
    err = np.abs(got - ref)
    bad = err > d
    assert not bad.any(), (name, int(bad.sum()), float(err[bad].max()), float(d[bad].min()))
    pos = d > 0
    worst[name] = float((err[pos] / d[pos]).max()) if pos.any() else 0.0


def _parts(t, stride):
    from wgsr import _lib
    return _lib.load().wgsr_droid_be_parts(t.shape[2], t.shape[3], stride)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("norm", NORMS)
def test_every_launch_against_the_oracle_on_the_stored_inputs(norm, shape):
    c = _case(norm, shape)
    P, g = c["P"], c["inter"]
    inst = norm == "instance"
    worst = {}
    raw = lambda k: _np(g[k])  # noqa: E731
    st = lambda k: tuple(_np(g["S" + k[1:]])[..., i] for i in (0, 1)) if inst else None  # noqa: E731

    def check_stats(k, stride=1):
        if inst:
            mean, rstd, d_mean, d_rstd = br.stats(raw(k), _parts(g[k], stride))
            _within(g["S" + k[1:]][..., 0], mean, d_mean, worst, "mean " + k)
            _within(g["S" + k[1:]][..., 1], rstd, d_rstd, worst, "rstd " + k)

    R0, d = br.stem(c["images"], *P["conv1"])
    _within(g["R0"], R0, d, worst, "R0")
    check_stats("R0")
    a = da = None
    for name, src, second, side, stride, dst in br.LAUNCHES + (br.HEAD + (None, 1, None),):
        is_raw = second is not None and second.startswith("Rd")
        a, da = br.stage(raw(src), st(src), raw(second) if second else None, st(second) if is_raw else None)
        if side:
            _within(g[side], a, da, worst, side)
        if dst is None:
            break
        R, d = br.conv(a, da, *br.launch_weights(P, name, stride)[:2], stride, *br.launch_weights(P, name, stride)[2:])
        if stride == 2:
            half = R.shape[1] // 2
            _within(g[dst], R[:, :half], d[:, :half], worst, dst)
            _within(g["Rd" + dst[1:]], R[:, half:], d[:, half:], worst, "Rd" + dst[1:])
            check_stats("Rd" + dst[1:], 2)
        else:
            _within(g[dst], R, d, worst, dst)
        check_stats(dst, stride)
    res, d = br.head(a, da, *P["conv2"], norm)
    if inst:
        _within(c["gpu"][0], res, d, worst, "out")
    else:
        _within(c["gpu"][0], res[0], d[0], worst, "net")
        _within(c["gpu"][1], res[1], d[1], worst, "inp")
        assert bool((c["gpu"][0].abs() <= 1).all()) and bool((c["gpu"][0] < 0).any())      # tanh
        assert bool((c["gpu"][1] >= 0).all()) and bool((c["gpu"][1] == 0).any())            # relu
    top = max(worst, key=worst.get)
    print(f"\n{norm} {shape}: worst GPU error / bound over {len(worst)} maps: {worst[top]:.4f} ({top}); "
          f"statistics: {max([v for k, v in worst.items() if k[:4] in ('mean', 'rstd')] or [0]):.4f}")


def _rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("norm", NORMS)
def test_end_to_end_against_the_plain_float64_evaluation(norm, shape):
    c = _case(norm, shape)
    ratios = []
    for got, plain, rounded in zip(c["gpu"], _outputs(norm, c["plain"]), _outputs(norm, c["rounded"])):
        e16 = _rms(rounded - plain)
        ratios.append(_rms(_np(got) - plain) / e16)
    print(f"\n{norm} {shape}: rms(GPU - float64) / E16 = " + ", ".join(f"{r:.3f}" for r in ratios))
    assert max(ratios) <= 2.0, ratios


@pytest.mark.parametrize("tag", ["f", "c"])
def test_end_to_end_against_the_recorded_reference(tag):
    c = br.fixture_case(tag)
    norm = c["norm"]
    got, _ = _run(norm, torch.from_numpy(c["images"]).cuda(), _state_dict(c["P"]))
    z = c["z"]
    refs = (z["f_out"],) if tag == "f" else (np.tanh(z["c_out"][:, :128]), np.maximum(z["c_out"][:, 128:], 0))
    ratios = []
    for g, ref, plain, rounded in zip(got, refs, _outputs(norm, c["plain"]), _outputs(norm, c["rounded"])):
        ratios.append(_rms(_np(g) - ref) / _rms(rounded - plain))
    print(f"\nfixture {tag}: rms(GPU - recorded reference) / E16 = " + ", ".join(f"{r:.3f}" for r in ratios))
    assert max(ratios) <= 2.0, ratios


@pytest.mark.parametrize("norm", NORMS)
def test_frames_runs_and_call_forms_give_the_same_bits(norm):
    from wgsr import frontend
    shape = SHAPES[2]
    c = _case(norm, shape)
    x, g = c["dev"], c["gpu"]
    n, H, W = shape
    again, _ = _run(norm, x, c["params"])                                   # two runs
    assert all(torch.equal(a, b) for a, b in zip(again, g))
    for e in range(n):                                                      # each frame alone
        alone, _ = _run(norm, x[e:e + 1], c["params"])
        assert all(torch.equal(a, b[e:e + 1]) for a, b in zip(alone, g)), e
    ws = frontend.BasicEncoderWorkspace(n, H, W, norm, "cuda")              # the workspace form, twice
    for _ in range(2):
        got, inter = _run(norm, x, c["params"], workspace=ws, return_intermediates=True)
        assert all(torch.equal(a, b) for a, b in zip(got, g))
        assert sorted(inter) == sorted(c["inter"])
        for k, v in inter.items():
            assert torch.equal(v, c["inter"][k]), k
    assert inter["R5"].data_ptr() == ws.maps["R5"].data_ptr()               # (views of the workspace)
    f = frontend.feature_encoder if norm == "instance" else frontend.context_encoder
    out = f(x[None], c["sd"])                                               # the reference's call form, new buffers
    out = (out,) if norm == "instance" else out
    assert all(o.shape == b.shape and o.dtype == torch.float16 and torch.equal(o, b) for o, b in zip(out, g))
    half, _ = _run(norm, x.half(), c["params"])                             # float16 images of the same values
    assert all(torch.equal(a, b) for a, b in zip(half, g))


def test_outputs_beyond_the_receptive_field_of_the_border_are_unchanged():
    """cnet (with the instance norm every output depends on every pixel).  The receptive field of an output pixel is
    107 x 107 input pixels around (8 y, 8 x): 7 for the stem, 4 x 4 more for layer1 (steps of 2), 4 + 3 x 8 for layer2
    (steps of 4 after its first convolution), 8 + 3 x 16 for layer3.  In 1 x 120 x 136 with another outermost ring
    of pixels, the outputs with 8 y - 53 >= 1, 8 y + 53 <= 118, 8 x - 53 >= 1 and 8 x + 53 <= 134 keep their bits, and
    others change."""
    from wgsr import frontend
    c = _case("none", SHAPES[0])
    H, W = 120, 136
    gen = torch.Generator(device="cuda").manual_seed(8)
    x = torch.randn(1, 3, H, W, device="cuda", generator=gen).half().float()
    y = x.clone()
    y[:, :, 0], y[:, :, -1], y[:, :, :, 0], y[:, :, :, -1] = 3.0, -3.0, 2.0, -2.0
    a, b = (frontend.context_encoder(t, c["params"]) for t in (x, y))
    ys = [v for v in range(15) if 8 * v - 53 >= 1 and 8 * v + 53 <= H - 2]
    xs = [v for v in range(17) if 8 * v - 53 >= 1 and 8 * v + 53 <= W - 2]
    assert ys == [7, 8] and xs == [7, 8, 9, 10]
    for p, q in zip(a, b):
        assert torch.equal(p[:, :, 7:9, 7:11], q[:, :, 7:9, 7:11])
        assert not torch.equal(p[:, :, 6], q[:, :, 6]) and not torch.equal(p[:, :, :, 11], q[:, :, :, 11])


def _conv_launch(r, st, p, pst, side, stride, w3, w1, bias, parts=None):
    """wgsr_droid_be_conv on its own, epilogue raw -> out [n, rows3 + rows1, ho, wo] in a guarded buffer"""
    from wgsr import _lib
    n, c_in, hi, wi = r.shape
    rows3 = 0 if w3 is None else w3.shape[0]
    rows1 = 0 if w1 is None else w1.shape[0]
    dev_w3 = None if w3 is None else _pack3(w3)
    dev_w1 = None if w1 is None else _pack1(w1)
    ho, wo = ((hi + 1) // 2, (wi + 1) // 2) if stride == 2 else (hi, wi)
    whole, out = _guarded((n, rows3 + rows1, ho, wo))
    L = _lib.load()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    fs = lambda t: 0 if t is None else t.stride(0)  # noqa: E731
    _lib.check(L.wgsr_droid_be_conv(r.data_ptr(), r.stride(0), ptr(st), fs(st), ptr(p), fs(p), ptr(pst), fs(pst),
                                    ptr(side), c_in, stride, ptr(dev_w3), rows3, ptr(dev_w1), rows1, bias.data_ptr(),
                                    0, out.data_ptr(), None, ptr(parts), n, hi, wi,
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((whole[-GUARD:] == FILL).all()) and not bool((out == FILL).any())
    return out


def _pack3(w):
    from wgsr import frontend
    t = torch.from_numpy(w).cuda()
    return frontend._pack_layout(t.half(), torch.zeros(w.shape[0], device="cuda"))[0]


def _pack1(w):
    from wgsr import frontend
    t = torch.from_numpy(w).cuda()
    return frontend._conv1x1_layout(t, torch.zeros(w.shape[0], device="cuda"), t.device)[0]


@pytest.mark.parametrize("stride", [1, 2])
def test_padding_is_zero_after_the_transformation(stride):
    """A raw map of 19 x 27 whose channel 5 is the constant -100 with statistics (mean, rstd) = (-100, 1): form A
    stages ReLU(0) = 0 inside the map, and N(0) = +100 would appear outside it if the kernel padded the raw map.
    Channel 9 is the constant 3 with (1, 2): it stages 4 inside and 0 outside.  A 3 x 3 convolution of ones on one
    channel counts the taps inside the map: exactly 0 for channel 5, 4 x (9, 6 or 4 at stride 1) for channel 9.  The
    side output is the staged map."""
    n, C, hi, wi = 2, 32, 19, 27
    gen = torch.Generator(device="cuda").manual_seed(19)
    r = torch.randn(n, C, hi, wi, device="cuda", generator=gen).half()
    r[:, 5], r[:, 9] = -100.0, 3.0
    st = torch.zeros(n, C, 2, device="cuda")
    st[..., 1] = 1.0
    st[:, 5, 0], st[:, 9, 0], st[:, 9, 1] = -100.0, 1.0, 2.0
    w3 = np.zeros((32, C, 3, 3), np.float16)
    w3[0, 5], w3[17, 9] = 1.0, 1.0
    side = torch.full_like(r, FILL) if stride == 1 else None
    out = _conv_launch(r, st, None, None, side, stride, w3, None, torch.zeros(32, device="cuda"))
    inside = np.pad(np.ones((hi, wi)), 1)
    taps = sum(inside[ky:ky + hi, kx:kx + wi] for ky in range(3) for kx in range(3))[::stride, ::stride]
    assert {4.0, 6.0, 9.0} >= set(np.unique(taps)) and taps.min() == 4.0
    got = out.cpu().numpy()
    assert not got[:, 0].any()
    assert np.array_equal(got[:, 17], np.broadcast_to(4.0 * taps, got[:, 17].shape))
    assert not np.delete(got, (0, 17), axis=1).any()
    if side is not None:
        want = torch.relu((r.float() - st[..., 0, None, None]) * st[..., 1, None, None]).half()
        assert torch.equal(side, want) and not bool(side[:, 5].any()) and bool((side[:, 9] == 4).all())


def test_one_hot_stem_against_the_taps():
    """stem weights one-hot on (row, ci, ky, kx), bias 0: out[row](y, x) = fp16(image)[ci, 2 y - 3 + ky, 2 x - 3 + kx],
    zero outside the image; picks at the corners and the centre of the window and in the padded K-step, on an odd
    image with partial tiles.  The float32 image is not representable in float16: round to nearest even."""
    from wgsr import _lib, frontend
    n, H, W = 2, 37, 53
    rng = np.random.default_rng(37)
    img = rng.uniform(-4, 4, (n, 3, H, W)).astype(np.float32)
    img[0, 2, 0, :2] = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]     # ties
    img16 = img.astype(np.float16)
    assert img16[0, 2, 0, :2].tolist() == [1.0, 1.0 + 2.0 ** -9]
    picks = {0: (0, 0, 0), 5: (2, 6, 6), 16: (1, 3, 3), 31: (2, 0, 6), 20: (0, 6, 0)}    # row -> (ci, ky, kx)
    w = np.zeros((32, 3, 7, 7), np.float16)
    for row, (ci, ky, kx) in picks.items():
        w[row, ci, ky, kx] = 1.0
    pw, pb = frontend.pack_stem7x7(torch.from_numpy(w).cuda(), torch.zeros(32, device="cuda"))
    ho, wo = (H + 1) // 2, (W + 1) // 2
    whole, out = _guarded((n, 32, ho, wo))
    _lib.check(_lib.load().wgsr_droid_be_stem(torch.from_numpy(img).cuda().data_ptr(), 0, None, None, pw.data_ptr(),
                                              pb.data_ptr(), out.data_ptr(), None, n, H, W,
                                              torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((whole[-GUARD:] == FILL).all())
    got = out.cpu().numpy()
    pad = np.pad(img16, ((0, 0), (0, 0), (3, 5), (3, 5)))
    for row in range(32):
        if row not in picks:
            assert not got[:, row].any(), row
            continue
        ci, ky, kx = picks[row]
        want = pad[:, ci, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2]
        assert want.any() and np.array_equal(got[:, row], want), row


def test_one_hot_one_by_one_convolutions_against_the_taps():
    """the head (stride 1, 128 channels) and a downsample (stride 2, 32 channels, stacked under a zero 3 x 3) with
    one-hot weights: out[row] = ReLU(R[channel]) at (y, x), or at (2 y, 2 x) -- the centre tap of the staged tile"""
    gen = torch.Generator(device="cuda").manual_seed(41)
    r = torch.randn(2, 128, 5, 7, device="cuda", generator=gen).half()
    picks = {0: 127, 77: 0, 255: 64}
    w1 = np.zeros((256, 128, 1, 1), np.float16)
    for row, ch in picks.items():
        w1[row, ch] = 1.0
    out = _conv_launch(r, None, None, None, None, 1, None, w1, torch.zeros(256, device="cuda"))
    for row in range(256):
        want = torch.relu(r[:, picks[row]]) if row in picks else torch.zeros_like(r[:, 0])
        assert torch.equal(out[:, row], want), row
    r = torch.randn(2, 32, 19, 27, device="cuda", generator=gen).half()
    picks = {0: 31, 13: 0, 31: 17}
    w1 = np.zeros((32, 32, 1, 1), np.float16)
    for row, ch in picks.items():
        w1[row, ch] = 1.0
    out = _conv_launch(r, None, None, None, None, 2, np.zeros((32, 32, 3, 3), np.float16), w1,
                       torch.zeros(64, device="cuda"))
    assert out.shape == (2, 64, 10, 14) and not bool(out[:, :32].any())
    for row in range(32):
        want = torch.relu(r[:, picks[row], ::2, ::2]) if row in picks else torch.zeros_like(out[:, 0])
        assert torch.equal(out[:, 32 + row], want), row


@pytest.mark.parametrize("norm", NORMS)
def test_mean_and_std_equal_a_normalised_image_rounded_to_float16(norm):
    c = _case(norm, SHAPES[1])
    n, H, W = SHAPES[1]
    rng = np.random.default_rng(53)
    img = (rng.integers(0, 256, (n, 3, H, W)) / 255.0).astype(np.float32)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    pre = br.normalise_image(img, mean, std)
    assert not np.array_equal(pre, (img - np.float32(mean).reshape(1, 3, 1, 1)) / np.float32(std).reshape(1, 3, 1, 1))
    want, _ = _run(norm, torch.from_numpy(pre).cuda(), c["params"])
    got, _ = _run(norm, torch.from_numpy(img).cuda(), c["params"], mean=mean, std=torch.tensor(std, device="cuda"))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    raw, _ = _run(norm, torch.from_numpy(img).cuda(), c["params"])
    assert not torch.equal(raw[0], want[0])


@pytest.mark.parametrize("norm", NORMS)
def test_the_call_replays_from_one_graph_to_the_same_bits(norm):
    from wgsr import frontend
    shape = SHAPES[1]
    c = _case(norm, shape)
    ws = frontend.BasicEncoderWorkspace(*shape, norm, "cuda")
    outs = tuple(torch.full_like(g, FILL) for g in c["gpu"])
    f = frontend.feature_encoder if norm == "instance" else frontend.context_encoder
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f(c["dev"], c["params"], out=outs[0] if norm == "instance" else outs, workspace=ws)
    for _ in range(2):
        for t in outs + tuple(ws.maps.values()) + tuple(ws.stats.values()):
            t.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, c["gpu"]))
        for k, v in ws.named().items():
            assert torch.equal(v, c["inter"][k]), k


def test_argument_errors():
    from wgsr import frontend
    shape = SHAPES[0]
    n, H, W = shape
    for norm, f in (("instance", frontend.feature_encoder), ("none", frontend.context_encoder)):
        c = _case(norm, shape)
        x, p = c["dev"], c["params"]
        with pytest.raises(NotImplementedError, match="float32 or float16"):
            f(x.double(), p)
        with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
            f(x.cpu(), p)
        with torch.enable_grad():
            with pytest.raises(NotImplementedError, match="images requires grad"):
                f(x.clone().requires_grad_(), p)
        with pytest.raises(ValueError, match="images must be"):
            f(x[:, :2].contiguous(), p)
        with pytest.raises(ValueError, match="images must be contiguous"):
            f(x.repeat(1, 1, 1, 2)[..., ::2], p)
        with pytest.raises(ValueError, match="must be a contiguous"):
            bad = torch.empty(n, 64, 2, 3, dtype=torch.float16, device="cuda")
            f(x, p, out=bad if norm == "instance" else (bad, bad))
        with pytest.raises(ValueError, match="workspace: made for"):
            f(x, p, workspace=frontend.BasicEncoderWorkspace(n, H, W + 8, norm, "cuda"))
        with pytest.raises(ValueError, match="mean and std"):
            f(x, p, mean=[0.0, 0.0, 0.0])
        other = _case("none" if norm == "instance" else "instance", shape)["params"]
        with pytest.raises(ValueError, match="params were packed with norm"):
            f(x, other)
        e = f(x[:0], p)                                                     # no images: empty results
        e = (e,) if norm == "instance" else e
        assert all(t.shape == (0, 128, 2, 3) and t.dtype == torch.float16 for t in e)
    c = _case("instance", shape)
    with pytest.raises(ValueError, match="one pixel"):                      # torch raises too
        frontend.feature_encoder(c["dev"][:, :, :8, :8].contiguous(), c["params"])
    one, _ = _run("none", _case("none", shape)["dev"][:, :, :8, :8].contiguous(), _case("none", shape)["params"])
    assert one[0].shape == (n, 128, 1, 1)
    with pytest.raises(RuntimeError, match="wgsr_droid_be_conv"):           # the entry point's own checks
        r = torch.zeros(1, 96, 4, 4, dtype=torch.float16, device="cuda")
        _conv_launch(r, None, None, None, None, 1, np.zeros((32, 96, 3, 3), np.float16), None,
                     torch.zeros(32, device="cuda"))
