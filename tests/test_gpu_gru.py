"""GPU tests of the update operator's ConvGRU on the wide-K fp16 MFMA 3 x 3
convolution (csrc/droid_gru.hip; wgsr.frontend.conv_gru) against the float64
oracle tests/_gru_ref.py and the recorded outputs of the reference's own module
(tests/golden/ref_gru.npz).

Shapes n x ht x wd: 2 x 3 x 5 (every pixel at a border, smaller than any tile),
3 x 9 x 17 (partial tiles both ways, one tile of a single column), 2 x 8 x 16
(whole tiles), 1 x 48 x 64 (the tracker's map).  Inputs are standard normal
rounded to float16, 3 x 3 weights scaled by 1 / sqrt(4032) and 1 x 1 weights by
1 / sqrt(128).

The bound of every output element is the oracle's ``d`` (first-order
propagation of the fp32 accumulation, of the fp32 activations and of the three
float16 rounding points; see tests/_gru_ref.py), ``d + r`` against the recorded
float64 reference, and the tighter per-stage ``d`` where a stage is evaluated
on the kernel's own intermediates.  Nothing is fitted to the kernel.  Each test
prints its worst error / bound ratio.  Every output and scratch buffer is a
guarded one (FILL / GUARD).
"""
import numpy as np
import pytest
import torch

import _gru_ref as gr

pytestmark = pytest.mark.gpu

FILL = -7.0
GUARD = 64
SHAPES = [(2, 3, 5), (3, 9, 17), (2, 8, 16), (1, 48, 64)]
OUTPUTS = ("gbias", "z", "rnet", "out")
_cache = {}


def _ids(s):
    return "x".join(map(str, s))


def _state_dict(P, prefix="update.gru."):
    sd = {}
    for name, (w, b) in P.items():
        sd[f"{prefix}{name}.weight"] = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        sd[f"{prefix}{name}.bias"] = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    return sd


def _guarded(shape, dtype):
    """(a tensor of `shape` filled with FILL, the buffer it is the head of: GUARD more elements follow)"""
    whole = torch.full((int(np.prod(shape)) + GUARD,), FILL, dtype=dtype, device="cuda")
    return whole[:-GUARD].view(shape), whole


def _run(net, inp, corr, flow, params, **kw):
    """conv_gru into guarded buffers -> (dict of gbias, z, rnet, out on the device, the whole buffers of these
    and of the glo term's partial sums)"""
    from wgsr import frontend
    n, ht, wd = net.shape[-4], net.shape[-2], net.shape[-1]
    bufs = {"gbias": _guarded((n, 384), torch.float32)}
    for k in ("z", "rnet", "out"):
        bufs[k] = _guarded((n, 128, ht, wd), torch.float16)
    bufs["part"] = _guarded((n, (ht * wd + 127) // 128, 128), torch.float32)    # the glo term's partial sums
    wholes = [bufs[k][1] for k in OUTPUTS + ("part",)]
    try:
        got, mid = frontend.conv_gru(net, inp, corr, flow, params, out=bufs["out"][0], return_intermediates=True,
                                     scratch=tuple(bufs[k][0] for k in ("gbias", "z", "rnet", "part")), **kw)
    except RuntimeError as err:
        err.wholes = wholes
        raise
    assert got is bufs["out"][0] and all(mid[k] is bufs[k][0] for k in ("gbias", "z", "rnet"))
    for w in wholes:
        assert bool((w[-GUARD:] == FILL).all())
    return {k: bufs[k][0] for k in OUTPUTS}, wholes


def _case(shape):
    """inputs, parameters, the end-to-end oracle and the GPU's results of one shape, computed once and shared
    (never modified)"""
    if shape in _cache:
        return _cache[shape]
    from wgsr import frontend
    n, ht, wd = shape
    rng = np.random.default_rng(1000 * n + 10 * ht + wd)
    P = gr.make_params(rng)
    x = dict(zip(("net", "inp", "corr", "flow"), gr.make_inputs(rng, n, ht, wd)))
    sd = _state_dict(P)
    c = {"P": P, "x": x, "sd": sd, "params": frontend.UpdateGRU.from_state_dict(sd),
         "oracle": gr.gru(x["net"], x["inp"], x["corr"], x["flow"], P),
         "dev": {k: torch.from_numpy(v).cuda() for k, v in x.items()}}
    d = c["dev"]
    c["gpu"], _ = _run(d["net"], d["inp"], d["corr"], d["flow"], c["params"])
    c["host"] = {k: v.cpu().numpy().astype(np.float64) for k, v in c["gpu"].items()}
    _cache[shape] = c
    return c


def _ratio(got, ref, bound):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_conv_gru_against_oracle(shape):
    c = _case(shape)
    o = c["oracle"]
    worst = {k: _ratio(c["host"][k], o[k], o["d_" + k]) for k in OUTPUTS}
    print(f"\nconv_gru {shape}: worst GPU error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    z = c["host"]["z"]
    assert ((z >= 0) & (z <= 1)).all() and 0.2 < z.mean() < 0.8


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_each_stage_on_the_kernels_own_intermediates(shape):
    """stage_zr fed the GPU's gbias, stage_q fed the GPU's rnet, z and gbias: exactly known inputs, so the
    bound of a stage is that of one convolution, its activation and one float16 rounding"""
    c = _case(shape)
    x, h, P = c["x"], c["host"], c["P"]
    zr = gr.stage_zr(x["net"], x["inp"], x["corr"], x["flow"], h["gbias"], P)
    q = gr.stage_q(h["rnet"], x["inp"], x["corr"], x["flow"], h["gbias"], h["z"], x["net"], P)
    worst = {"z": _ratio(h["z"], zr["z"], zr["d_z"]), "rnet": _ratio(h["rnet"], zr["rnet"], zr["d_rnet"]),
             "out": _ratio(h["out"], q["out"], q["d_out"])}
    print(f"\nconv_gru stages {shape}: worst GPU error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    assert (q["d_out"] <= c["oracle"]["d_out"]).all() and (zr["d_z"] <= c["oracle"]["d_z"]).all()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_recorded_reference_outputs(tag):
    """the reference's own ConvGRU, run in float64 without any rounding point: within d + r"""
    c = gr.fixture_case(tag)
    o = gr.gru(c["net"], c["inp"], c["corr"], c["flow"], c["P"])
    dev = [torch.from_numpy(c[k]).cuda() for k in ("net", "inp", "corr", "flow")]
    got, _ = _run(*dev, _state_dict(c["P"]))
    worst = {}
    for name in OUTPUTS:
        rows = gr.FIXTURE_ZR_ROWS if name in ("z", "rnet") else slice(None)
        rec = c["z"][f"{tag}_" + ("net_out" if name == "out" else name)]
        g = got[name].cpu().numpy()
        worst[name] = _ratio(g[:, rows] if g.ndim == 4 else g, rec,
                             (o["d_" + name] + o["r_" + name])[:, rows] if g.ndim == 4 else o["d_" + name])
    print(f"\nfixture {tag}: worst GPU error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def _with(P, **changes):
    """P with the named parameters replaced: name=(weight or None, bias or None), None keeps the entry"""
    Q = dict(P)
    for name, (w, b) in changes.items():
        Q[name] = (P[name][0] if w is None else w, P[name][1] if b is None else b)
    return Q


def _zeros_w(P, name):
    return np.zeros_like(P[name][0])


def _const_b(v):
    return np.full(128, v, np.float32)


def test_a_closed_update_gate_returns_net_and_an_open_one_q():
    """convz zero with bias -30: z rounds to 0 and net' is net, bit for bit.  With bias +30: z is 1 and net' the
    float16 rounding of q, which the q stage's oracle gives on the GPU's own rnet."""
    c = _case(SHAPES[1])
    d, x = c["dev"], c["x"]
    closed = _with(c["P"], convz=(_zeros_w(c["P"], "convz"), _const_b(-30.0)))
    got, _ = _run(d["net"], d["inp"], d["corr"], d["flow"], _state_dict(closed))
    assert not got["z"].any() and torch.equal(got["out"], d["net"])
    opened = _with(c["P"], convz=(_zeros_w(c["P"], "convz"), _const_b(30.0)))
    got, _ = _run(d["net"], d["inp"], d["corr"], d["flow"], _state_dict(opened))
    assert (got["z"] == 1).all()
    h = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}
    q = gr.stage_q(h["rnet"], x["inp"], x["corr"], x["flow"], h["gbias"], h["z"], x["net"], opened)
    assert np.array_equal(q["out"], gr.round_fp16(q["q"]))       # the oracle's net' is fp16(q)
    ratio = _ratio(h["out"], q["out"], q["d_out"])
    print(f"\nopen gate: worst |net' - fp16(q)| / bound {ratio:.4f}")
    assert ratio <= 1.0


def test_zero_w_gives_half_the_mean_of_net():
    """w zero (weights and bias): sigmoid(0) is exactly 0.5, so gbias = bias + conv_glo (0.5 mean(net)) + glo bias,
    within the bounds of the fp32 mean and of the 128-term products"""
    c = _case(SHAPES[1])
    d, x = c["dev"], c["x"]
    P = _with(c["P"], w=(_zeros_w(c["P"], "w"), _const_b(0.0)))
    got, _ = _run(d["net"], d["inp"], d["corr"], d["flow"], _state_dict(P))
    n, _, ht, wd = x["net"].shape
    HW = ht * wd
    u = 0.5 * x["net"].astype(np.float64).reshape(n, 128, HW)
    glo, dglo = u.mean(axis=2), (HW + 2) * gr.U32 * np.abs(u).mean(axis=2)
    worst = 0.0
    for k, name in enumerate(gr.GATES):
        wg, bg = P[name + "_glo"][0].astype(np.float64).reshape(128, 128), P[name + "_glo"][1].astype(np.float64)
        bk = P[name][1].astype(np.float64)
        ref = bk[None] + glo @ wg.T + bg[None]
        bound = (128 + 3) * gr.U32 * (np.abs(glo) @ np.abs(wg).T + np.abs(bk) + np.abs(bg)) + dglo @ np.abs(wg).T
        worst = max(worst, _ratio(got["gbias"][:, 128 * k:128 * k + 128].cpu().numpy(), ref, bound))
    print(f"\nzero w: worst gbias error / bound {worst:.4f}")
    assert worst <= 1.0


def test_one_hot_convq_reads_the_shifted_channel_of_each_source():
    """convq one-hot on (concatenated channel, tap) in a row, its bias and convq_glo zero, the update gate open:
    net'[row] = fp16(tanh(source channel shifted by the tap)), zero where that lies outside the map, and 0 in
    every other row.  Pins the concatenation order [rnet, inp, corr, flow], the 64-channel last chunk (channel
    447 included) and the halo (corner taps)."""
    c = _case(SHAPES[1])
    d, P0 = c["dev"], c["P"]
    n, ht, wd = SHAPES[1]
    picks = {5: (37, 4), 20: (128 + 70, 1), 64: (256 + 127, 7), 100: (384 + 10, 3), 127: (447, 0), 33: (0, 8)}
    wq = _zeros_w(P0, "convq")
    for row, (ch, tap) in picks.items():
        wq[row, ch, tap // 3, tap % 3] = 1.0
    P = _with(P0, convz=(_zeros_w(P0, "convz"), _const_b(30.0)), convq=(wq, _const_b(0.0)),
              convq_glo=(_zeros_w(P0, "convq_glo"), _const_b(0.0)))
    got, _ = _run(d["net"], d["inp"], d["corr"], d["flow"], _state_dict(P))
    assert not got["gbias"][:, 256:].any() and (got["z"] == 1).all()
    cat = torch.cat([got["rnet"], d["inp"], d["corr"], d["flow"]], dim=1).cpu().numpy().astype(np.float64)
    pad = np.pad(cat, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = got["out"].cpu().numpy().astype(np.float64)
    worst = 0.0
    for row in range(128):
        if row not in picks:
            assert not out[:, row].any(), row
            continue
        ch, tap = picks[row]
        want = np.tanh(pad[:, ch, tap // 3:tap // 3 + ht, tap % 3:tap % 3 + wd])
        assert np.abs(want).max() > 0.5
        bound = gr.TANH_ABS + gr.ulp_fp16(np.abs(want) + gr.TANH_ABS)
        worst = max(worst, _ratio(out[:, row], gr.round_fp16(want), bound))
    print(f"\none-hot convq: worst |net' - fp16(tanh(shifted input))| / bound {worst:.4f}")
    assert worst <= 1.0


def test_runs_edges_index_and_call_forms_give_the_same_bits():
    from wgsr import frontend
    c = _case(SHAPES[1])
    d, g = c["dev"], c["gpu"]
    n = SHAPES[1][0]
    args = (d["net"], d["inp"], d["corr"], d["flow"])
    again, _ = _run(*args, c["params"])                                  # two runs
    for k in OUTPUTS:
        assert torch.equal(again[k], g[k]), k
    for e in range(n):                                                   # each edge alone
        one, _ = _run(*(t[e:e + 1] for t in args), c["params"])
        for k in OUTPUTS:
            assert torch.equal(one[k], g[k][e:e + 1]), (e, k)
    # inp as the frame buffer with a non-monotone index that repeats a frame, against the gathered copy
    gen = torch.Generator(device="cuda").manual_seed(3)
    inps = torch.randn(4, 128, *SHAPES[1][1:], device="cuda", generator=gen).half()
    ix = torch.tensor([2, 0, 2], device="cuda")
    gathered, _ = _run(d["net"], inps[ix].contiguous(), d["corr"], d["flow"], c["params"])
    indexed, _ = _run(d["net"], inps, d["corr"], d["flow"], c["params"], inp_ix=ix)
    assert not torch.equal(gathered["out"], g["out"])
    for k in OUTPUTS:
        assert torch.equal(indexed[k], gathered[k]), k
    # the reference's call form (a leading batch dimension, the state_dict itself), new buffers
    out = frontend.conv_gru(d["net"][None], d["inp"][None], d["corr"][None], d["flow"][None], c["sd"])
    assert out.shape == g["out"].shape and out.dtype == torch.float16 and torch.equal(out, g["out"])
    bare = frontend.conv_gru(*args, _state_dict(c["P"], prefix=""))
    assert torch.equal(bare, g["out"])


def test_every_cu_busy_gives_the_bits_of_single_edge_calls():
    """24 edges of 48 x 64: 576 workgroups of 16 x 8 tiles in the q launch and 1152 in the zr launch, more than
    two per CU; each edge bit for bit what a call with that edge alone gives"""
    from wgsr import frontend
    c = _case(SHAPES[3])
    n, ht, wd = 24, 48, 64
    gen = torch.Generator(device="cuda").manual_seed(24)
    net, inp, corr = (torch.randn(n, 128, ht, wd, device="cuda", generator=gen).half() for _ in range(3))
    flow = torch.randn(n, 64, ht, wd, device="cuda", generator=gen).half()
    got, _ = _run(net, inp, corr, flow, c["params"])
    for e in range(n):
        s = slice(e, e + 1)
        out, mid = frontend.conv_gru(net[s], inp[s], corr[s], flow[s], c["params"], return_intermediates=True)
        assert torch.equal(out, got["out"][s]), e
        for k in ("gbias", "z", "rnet"):
            assert torch.equal(mid[k], got[k][s]), (e, k)


def test_unchecked_call_replays_from_a_graph_to_the_same_bits():
    from wgsr import frontend
    c = _case(SHAPES[2])
    d, p = c["dev"], c["params"]
    gen = torch.Generator(device="cuda").manual_seed(8)
    inps = torch.randn(3, 128, *SHAPES[2][1:], device="cuda", generator=gen).half()
    ix = torch.tensor([2, 0], device="cuda")
    eager = frontend.conv_gru(d["net"], inps, d["corr"], d["flow"], p, inp_ix=ix)
    torch.cuda.synchronize()
    bufs = [torch.full_like(c["gpu"]["out"], FILL) for _ in range(2)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frontend.conv_gru(d["net"], d["inp"], d["corr"], d["flow"], p, check=False, out=bufs[0])
        frontend.conv_gru(d["net"], inps, d["corr"], d["flow"], p, inp_ix=ix, check=False, out=bufs[1])
    for t in bufs:
        t.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], c["gpu"]["out"]) and torch.equal(bufs[1], eager)


def test_out_of_range_inp_ix_raises_and_writes_nothing():
    c = _case(SHAPES[2])
    d, p = c["dev"], c["params"]
    F = 3
    inps = d["inp"][:1].repeat(F, 1, 1, 1)
    for bad_value in (-1, F):
        ix = torch.tensor([1, bad_value], device="cuda")
        with pytest.raises(RuntimeError, match="outside") as info:
            _run(d["net"], inps, d["corr"], d["flow"], p, inp_ix=ix)
        assert "WGSR_GRU_BAD_IX" in str(info.value) and "nothing was written" in str(info.value)
        for whole in info.value.wholes:
            assert (whole == FILL).all()
        # unchecked: no exception, and still nothing written
        _, wholes = _run(d["net"], inps, d["corr"], d["flow"], p, inp_ix=ix, check=False)
        torch.cuda.synchronize()
        for whole in wholes:
            assert (whole == FILL).all()


def test_argument_errors():
    from wgsr import frontend
    c = _case(SHAPES[0])
    d, p = c["dev"], c["params"]
    n, ht, wd = SHAPES[0]
    net, inp, corr, flow = d["net"], d["inp"], d["corr"], d["flow"]
    with pytest.raises(NotImplementedError, match="autocast"):
        frontend.conv_gru(net.float(), inp, corr, flow, p)
    with pytest.raises(NotImplementedError, match="autocast"):
        frontend.conv_gru(net, inp, corr.float(), flow, p)
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.conv_gru(net.cpu(), inp, corr, flow, p)
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.conv_gru(net, inp, corr, flow.cpu(), p)
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="net requires grad"):
            frontend.conv_gru(net.clone().requires_grad_(), inp, corr, flow, p)
    with pytest.raises(ValueError, match="flow must be"):
        frontend.conv_gru(net, inp, corr, torch.zeros(n, 63, ht, wd, dtype=torch.float16, device="cuda"), p)
    with pytest.raises(ValueError, match="corr must be"):
        frontend.conv_gru(net, inp, torch.zeros(n, 128, ht + 1, wd, dtype=torch.float16, device="cuda"), flow, p)
    with pytest.raises(ValueError, match="net must be"):
        frontend.conv_gru(net[:, :64].contiguous(), inp, corr, flow, p)
    with pytest.raises(ValueError, match="inp must be contiguous"):
        frontend.conv_gru(net, torch.zeros(n, 128, ht, 2 * wd, dtype=torch.float16, device="cuda")[..., ::2], corr,
                          flow, p)
    with pytest.raises(ValueError, match="out must not overlap net"):
        frontend.conv_gru(net, inp, corr, flow, p, out=net)
    with pytest.raises(ValueError, match="entries of inp_ix"):
        frontend.conv_gru(net, inp, corr, flow, p, inp_ix=torch.zeros(n + 1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="inp must be"):   # without an index inp is per edge
        frontend.conv_gru(net, inp.repeat(2, 1, 1, 1), corr, flow, p)
    # the library's own check: scratch buffers that overlap each other
    z = torch.empty_like(net)
    with pytest.raises(RuntimeError, match="overlaps"):
        frontend.conv_gru(net, inp, corr, flow, p, scratch=(torch.empty(n, 384, device="cuda"), z, z))
    # no edges: nothing to do
    out = frontend.conv_gru(net[:0], inp[:0], corr[:0], flow[:0], p)
    assert out.shape == (0, 128, ht, wd) and out.dtype == torch.float16
