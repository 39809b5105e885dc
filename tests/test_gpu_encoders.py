"""GPU tests of the update operator's fused corr and flow encoders
(csrc/droid_encoders.hip; wgsr.frontend.corr_encoder / flow_encoder) against the
float64 oracle tests/_encoders_ref.py and the recorded outputs of the
reference's own modules (tests/golden/ref_encoders.npz).

Shapes n x ht x wd: 2 x 3 x 5 (smaller than any tile and than the 7 x 7 window:
every pixel at a border), 3 x 9 x 17 (partial tiles both ways, one tile of a
single column), 2 x 8 x 16 (whole tiles), 1 x 48 x 64 (the tracker's map).  corr
is standard normal rounded to float16, flow uniform in [-64, 64] rounded to
float16 and handed over as float32; weights scaled by 1 / sqrt(K).

The bound of every output element is the oracle's ``d`` (first-order
propagation of the two fp32 accumulations and of the two float16 rounding
points; see tests/_encoders_ref.py), ``d + r`` against the recorded float64
reference; the structural tests (padding of the hidden layer, one-hot first
layers, no read past channel 195, bit-identity) are exact.  Nothing is fitted to
the kernel.  Every output buffer is a guarded one (FILL / GUARD).
"""
import numpy as np
import pytest
import torch

import _encoders_ref as er

pytestmark = pytest.mark.gpu

FILL = -7.0
GUARD = 64
SHAPES = er.GPU_SHAPES
ENCODERS = ("corr", "flow")
C_OUT = {"corr": 128, "flow": 64}
_cache = {}


def _ids(s):
    return "x".join(map(str, s))


def _state_dict(P, prefix="update."):
    sd = {}
    for name, (w, b) in P.items():
        sd[f"{prefix}{name}.weight"] = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        sd[f"{prefix}{name}.bias"] = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    return sd


def _run(enc, x, params):
    """the encoder into a guarded buffer -> its output on the device"""
    from wgsr import frontend
    n, ht, wd = x.shape[-4], x.shape[-2], x.shape[-1]
    shape = (n, C_OUT[enc], ht, wd)
    whole = torch.full((int(np.prod(shape)) + GUARD,), FILL, dtype=torch.float16, device="cuda")
    out = whole[:-GUARD].view(shape)
    got = (frontend.corr_encoder if enc == "corr" else frontend.flow_encoder)(x, params, out=out)
    assert got is out and bool((whole[-GUARD:] == FILL).all())
    assert not bool((out == FILL).any())      # every element is written (no output is negative)
    return out


def _case(shape):
    """the shared oracle case of a shape (tests/_encoders_ref.shape_case) with the GPU's results, computed once"""
    if shape not in _cache:
        from wgsr import frontend
        c = dict(er.shape_case(shape))
        c["sd"] = _state_dict(c["P"])
        c["params"] = frontend.UpdateEncoders.from_state_dict(c["sd"])
        c["dev"] = {"corr": torch.from_numpy(c["corr_in"]).cuda(), "flow": torch.from_numpy(c["flow_in"]).cuda()}
        c["gpu"] = {enc: _run(enc, c["dev"][enc], c["params"]) for enc in ENCODERS}
        _cache[shape] = c
    return _cache[shape]


def _ratio(got, ref, bound):
    got = np.asarray(got.cpu().numpy() if torch.is_tensor(got) else got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / bound).max())


def _with(P, changes):
    """P with the named parameters replaced"""
    return {**P, **changes}


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_encoders_against_oracle(shape):
    c = _case(shape)
    worst = {enc: _ratio(c["gpu"][enc], c[enc]["out"], c[enc]["d_out"]) for enc in ENCODERS}
    print(f"\nencoders {shape}: worst GPU error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("tag", ["a", "b"])
def test_recorded_reference_outputs(tag):
    """the reference's own modules, run in float64 without any rounding point: within d + r"""
    c = er.fixture_case(tag)
    sd = _state_dict(c["P"])
    worst = {}
    for enc, f in (("corr", er.corr_encoder), ("flow", er.flow_encoder)):
        o = f(c[enc], c["P"])
        got = _run(enc, torch.from_numpy(c[enc]).cuda(), sd)
        worst[enc] = _ratio(got, c["z"][f"{tag}_{enc}_out"], o["d_out"] + o["r_out"])
    print(f"\nfixture {tag}: worst GPU error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("enc", ENCODERS)
def test_the_second_convolution_pads_the_hidden_layer(enc):
    """First-layer weight zero and bias 1 in one hidden channel: the hidden layer is 1 in that channel inside the
    map.  A one-hot second layer on (row, that channel, tap) then gives exactly 1 where the shifted pixel lies inside
    the map and exactly 0 outside (a first layer evaluated on a zero-padded input would give ReLU(bias) = 1
    there), and 0 in every other row.  A corner tap and an edge tap, on partial tiles."""
    shape = SHAPES[1]
    c = _case(shape)
    n, ht, wd = shape
    first, second = f"{enc}_encoder.0", f"{enc}_encoder.2"
    hidden_ch = 77
    b1 = np.zeros(128, np.float32)
    b1[hidden_ch] = 1.0
    picks = {3: 0, C_OUT[enc] - 1: 5}      # row -> tap: corner (0, 0), edge (1, 2)
    w2 = np.zeros_like(c["P"][second][0])
    for row, tap in picks.items():
        w2[row, hidden_ch, tap // 3, tap % 3] = 1.0
    P = _with(c["P"], {first: (np.zeros_like(c["P"][first][0]), b1), second: (w2, np.zeros(C_OUT[enc], np.float32))})
    got = _run(enc, c["dev"][enc], _state_dict(P)).cpu().numpy()
    inside = np.pad(np.ones((ht, wd), np.float16), 1)
    for row in range(C_OUT[enc]):
        if row not in picks:
            assert not got[:, row].any(), row
            continue
        ky, kx = divmod(picks[row], 3)
        want = inside[ky:ky + ht, kx:kx + wd]
        assert (want == 0).any() and (want == 1).any()
        assert np.array_equal(got[:, row], np.broadcast_to(want, (n, ht, wd))), row


def test_one_hot_first_layer_of_the_corr_encoder():
    """corr_encoder.0 one-hot on channels 0, 127, 128 and 195 (the last of each staged chunk's kind and the last
    real channel), the second layer the identity at the centre tap for that hidden channel: out[row] =
    fp16(ReLU(corr[channel])) -- exactly the ReLU of the float16 input"""
    c = _case(SHAPES[1])
    picks = {0: 0, 50: 127, 51: 128, 127: 195}    # hidden channel = row -> corr channel
    w1 = np.zeros_like(c["P"]["corr_encoder.0"][0])
    w2 = np.zeros_like(c["P"]["corr_encoder.2"][0])
    for row, ch in picks.items():
        w1[row, ch, 0, 0] = 1.0
        w2[row, row, 1, 1] = 1.0
    zero = np.zeros(128, np.float32)
    P = _with(c["P"], {"corr_encoder.0": (w1, zero), "corr_encoder.2": (w2, zero)})
    got = _run("corr", c["dev"]["corr"], _state_dict(P)).cpu().numpy()
    for row in range(128):
        if row not in picks:
            assert not got[:, row].any(), row
            continue
        want = np.maximum(c["corr_in"][:, picks[row]], np.float16(0))
        assert (want > 0).any() and np.array_equal(got[:, row], want), row


def test_one_hot_first_layer_of_the_flow_encoder_and_the_cast():
    """flow_encoder.0 one-hot on (channel, ky, kx) = (3, 0, 0), (3, 6, 6), (3, 3, 3) and (0, 0, 6), the second layer
    the identity at the centre tap: out[row] = fp16(ReLU(flow shifted by the tap)), zero where the tap leaves
    the map.  The float32 input is not representable in float16: the kernel's cast is round to nearest even
    (numpy's astype)."""
    shape = SHAPES[1]
    c = _case(shape)
    n, ht, wd = shape
    rng = np.random.default_rng(77)
    flow = rng.uniform(-64, 64, (n, 4, ht, wd)).astype(np.float32)
    flow[0, 3, 0, :4] = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2049.0, 2051.0]    # ties: to even
    flow16 = flow.astype(np.float16)
    assert not np.array_equal(flow16.astype(np.float32), flow)
    assert flow16[0, 3, 0, :4].tolist() == [1.0, 1.0 + 2.0 ** -9, 2048.0, 2052.0]
    picks = {0: (3, 0, 0), 17: (3, 6, 6), 64: (3, 3, 3), 127: (0, 0, 6)}    # hidden channel -> (ci, ky, kx)
    rows = {0: 0, 17: 1, 64: 2, 127: 63}                                    # hidden channel -> output row
    w1 = np.zeros_like(c["P"]["flow_encoder.0"][0])
    w2 = np.zeros_like(c["P"]["flow_encoder.2"][0])
    for h, (ci, ky, kx) in picks.items():
        w1[h, ci, ky, kx] = 1.0
        w2[rows[h], h, 1, 1] = 1.0
    P = _with(c["P"], {"flow_encoder.0": (w1, np.zeros(128, np.float32)),
                       "flow_encoder.2": (w2, np.zeros(64, np.float32))})
    got = _run("flow", torch.from_numpy(flow).cuda(), _state_dict(P)).cpu().numpy()
    pad = np.pad(flow16, ((0, 0), (0, 0), (3, 3), (3, 3)))
    seen = {row: h for h, row in rows.items()}
    for row in range(64):
        if row not in seen:
            assert not got[:, row].any(), row
            continue
        ci, ky, kx = picks[seen[row]]
        want = np.maximum(pad[:, ci, ky:ky + ht, kx:kx + wd], np.float16(0))
        assert (want > 0).any() and np.array_equal(got[:, row], want), row


def test_no_channel_past_195_is_read():
    """+inf in channels 0 .. 3 of edge 1 is what a read of channels 196 .. 199 of edge 0 would meet: edge 0 stays
    finite and bit-identical to the call with edge 0 alone (a zero weight does not neutralise an infinity)"""
    shape = SHAPES[0]
    c = _case(shape)
    corr = c["dev"]["corr"].clone()
    corr[1, :4] = float("inf")
    got = _run("corr", corr, c["params"])
    alone = _run("corr", corr[:1], c["params"])
    assert bool(torch.isfinite(got[0]).all()) and torch.equal(got[:1], alone)
    assert torch.equal(alone, c["gpu"]["corr"][:1])


def test_runs_edges_dtypes_and_call_forms_give_the_same_bits():
    from wgsr import frontend
    shape = SHAPES[1]
    c = _case(shape)
    for enc in ENCODERS:
        x, g = c["dev"][enc], c["gpu"][enc]
        assert torch.equal(_run(enc, x, c["params"]), g)                  # two runs
        for e in range(shape[0]):                                         # each edge alone
            assert torch.equal(_run(enc, x[e:e + 1], c["params"]), g[e:e + 1]), (enc, e)
        f = frontend.corr_encoder if enc == "corr" else frontend.flow_encoder
        out = f(x[None], c["sd"])                                         # the reference's call form, a new buffer
        assert out.shape == g.shape and out.dtype == torch.float16 and torch.equal(out, g)
        assert torch.equal(f(x, _state_dict(c["P"], prefix="")), g)
    assert c["dev"]["flow"].dtype == torch.float32
    assert torch.equal(_run("flow", c["dev"]["flow"].half(), c["params"]), c["gpu"]["flow"])    # fp16 flow


def test_every_cu_busy_gives_the_bits_of_single_edge_calls():
    """24 edges of 48 x 64: 576 workgroups per launch, more than two per CU; each edge bit for bit what a call with
    that edge alone gives"""
    c = _case(SHAPES[3])
    n, ht, wd = 24, 48, 64
    gen = torch.Generator(device="cuda").manual_seed(24)
    x = {"corr": torch.randn(n, 196, ht, wd, device="cuda", generator=gen).half(),
         "flow": 64 * torch.rand(n, 4, ht, wd, device="cuda", generator=gen) - 32}
    for enc in ENCODERS:
        got = _run(enc, x[enc], c["params"])
        for e in range(n):
            assert torch.equal(_run(enc, x[enc][e:e + 1], c["params"]), got[e:e + 1]), (enc, e)


def test_calls_replay_from_a_graph_to_the_same_bits():
    from wgsr import frontend
    c = _case(SHAPES[2])
    torch.cuda.synchronize()
    bufs = {enc: torch.full_like(c["gpu"][enc], FILL) for enc in ENCODERS}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frontend.corr_encoder(c["dev"]["corr"], c["params"], out=bufs["corr"])
        frontend.flow_encoder(c["dev"]["flow"], c["params"], out=bufs["flow"])
    for t in bufs.values():
        t.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    for enc in ENCODERS:
        assert torch.equal(bufs[enc], c["gpu"][enc]), enc


def test_argument_errors():
    from wgsr import frontend
    c = _case(SHAPES[0])
    p = c["params"]
    n, ht, wd = SHAPES[0]
    corr, flow = c["dev"]["corr"], c["dev"]["flow"]
    with pytest.raises(NotImplementedError, match="autocast"):
        frontend.corr_encoder(corr.float(), p)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        frontend.flow_encoder(flow.double(), p)
    for f, x in ((frontend.corr_encoder, corr), (frontend.flow_encoder, flow)):
        name = "corr" if x is corr else "flow"
        with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
            f(x.cpu(), p)
        with torch.enable_grad():
            with pytest.raises(NotImplementedError, match=f"{name} requires grad"):
                f(x.float().clone().requires_grad_(), p)
        with pytest.raises(ValueError, match=f"{name} must be"):
            f(x[:, :3].contiguous(), p)
        with pytest.raises(ValueError, match=f"{name} must be"):
            f(x[0, 0], p)
        with pytest.raises(ValueError, match=f"{name} must be contiguous"):
            f(x.repeat(1, 1, 1, 2)[..., ::2], p)
        with pytest.raises(ValueError, match="out must be"):
            f(x, p, out=torch.empty(n, 32, ht, wd, dtype=torch.float16, device="cuda"))
    # an out that overlaps the input: a buffer that holds both
    for f, ch, c_out in ((frontend.corr_encoder, 196, 128), (frontend.flow_encoder, 4, 64)):
        both = torch.zeros(n * (ch + c_out) * ht * wd, dtype=torch.float16, device="cuda")
        x = both[:n * ch * ht * wd].view(n, ch, ht, wd)
        out = both[n * ch * ht * wd - 8:-8].view(n, c_out, ht, wd)
        with pytest.raises(ValueError, match="out must not overlap"):
            f(x, p, out=out)
    # no edges: an empty float16 tensor
    e = frontend.corr_encoder(corr[:0], p)
    assert e.shape == (0, 128, ht, wd) and e.dtype == torch.float16
    e = frontend.flow_encoder(flow[:0], p)
    assert e.shape == (0, 64, ht, wd) and e.dtype == torch.float16
