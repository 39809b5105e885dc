"""GPU tests of the update operator's output heads on the fp16 MFMA 3 x 3
convolution (csrc/droid_conv3x3.hip; wgsr.frontend.conv3x3_relu / update_heads /
graph_agg) against the float64 oracle tests/_update_heads_ref.py and the
recorded outputs of the reference's own modules
(tests/golden/ref_update_heads.npz).

Shapes n x ht x wd: 3 x 3 x 5 (every pixel at a border, smaller than any tile),
4 x 9 x 11 (odd sizes, partial tiles in both directions), 5 x 8 x 16 (whole
tiles), 2 x 48 x 64 (the tracker's map).  Inputs are standard normal rounded to
float16, weights scaled by 1 / sqrt(1152).  Group patterns of graph_agg: a
non-monotone ``ii`` with a single-edge group (every shape), one group of 7
edges (9 x 3 x 5), and with a caller-given ``ix`` an empty group.

The bound of every output element is the oracle's ``d`` (first-order
propagation of the fp32 accumulation and of the float16 rounding points; see
tests/_update_heads_ref.py), and ``d + r`` against the recorded float64
reference.  Nothing is fitted to the kernel.  Each test prints its worst error /
bound ratio.
"""
import numpy as np
import pytest
import torch

import _update_heads_ref as hr

pytestmark = pytest.mark.gpu

FILL = -7.0
GUARD = 64
SHAPES = [(3, 3, 5), (4, 9, 11), (5, 8, 16), (2, 48, 64)]
II = {3: [4, 1, 4], 4: [7, 2, 7, 7], 5: [2, 0, 2, 5, 0], 2: [3, 0], 9: [1, 1, 4, 1, 1, 1, 0, 1, 1]}
_cache = {}


def _ids(s):
    return "x".join(map(str, s))


def _state_dict(P):
    sd = {}
    for name, (w, b) in P.items():
        sd[f"update.{name}.weight"] = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        sd[f"update.{name}.bias"] = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    return sd


def _case(shape):
    """inputs, parameters and oracles of one shape, computed once and shared (never modified)"""
    if shape in _cache:
        return _cache[shape]
    from wgsr import frontend
    n, ht, wd = shape
    rng = np.random.default_rng(1000 * n + 10 * ht + wd)
    P = hr.make_params(rng)
    net = rng.standard_normal((n, 128, ht, wd)).astype(np.float16)
    ii = np.asarray(II[n], np.int64)
    uniq, ix = np.unique(ii, return_inverse=True)
    sd = _state_dict(P)
    c = {"n": n, "ht": ht, "wd": wd, "P": P, "net": net, "ii": ii, "ix": ix, "G": len(uniq),
         "heads": hr.heads(net, P), "agg": hr.graph_agg(net, ix, len(uniq), P), "sd": sd,
         "params": frontend.UpdateHeads.from_state_dict(sd),
         "dev": {"net": torch.from_numpy(net).cuda(), "ii": torch.from_numpy(ii).cuda(),
                 "ix": torch.from_numpy(ix).cuda()}}
    _cache[shape] = c
    return c


def _guarded(shape, dtype):
    """(a tensor of `shape` filled with FILL, the buffer it is the head of: GUARD more elements follow)"""
    whole = torch.full((int(np.prod(shape)) + GUARD,), FILL, dtype=dtype, device="cuda")
    return whole[:-GUARD].view(shape), whole


def _guard_ok(whole):
    return bool((whole[-GUARD:] == FILL).all())


def _ratio(got, ref, bound):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_conv3x3_relu_against_oracle(shape):
    """the convolution alone (epilogue: bias, ReLU, one float16 rounding), 256 output rows"""
    from wgsr import frontend
    c = _case(shape)
    n, ht, wd = shape
    out, whole = _guarded((n, 256, ht, wd), torch.float16)
    got = frontend.conv3x3_relu(c["dev"]["net"], c["params"].hidden, out=out)
    assert got is out and _guard_ok(whole)
    ratio = _ratio(out, c["heads"]["hidden"], c["heads"]["d_hidden"])
    exact = float((out.cpu().numpy().astype(np.float64) == c["heads"]["hidden"]).mean())
    print(f"\nconv3x3_relu {shape}: worst GPU error / bound {ratio:.3f} (elements equal to the oracle's: {exact:.4f})")
    assert ratio <= 1.0
    # 128 rows (one pass), a new buffer, and bit-identical to the first 128 of the 256
    one = frontend.conv3x3_relu(c["dev"]["net"], frontend.pack_conv3x3(c["sd"]["update.delta.0.weight"],
                                                                      c["sd"]["update.delta.0.bias"]))
    assert one.shape == (n, 128, ht, wd) and torch.equal(one, out[:, :128])


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_update_heads_against_oracle(shape):
    from wgsr import frontend
    c = _case(shape)
    n, ht, wd = shape
    h = c["heads"]
    (delta, dwhole), (weight, wwhole) = _guarded((n, ht, wd, 2), torch.float32), _guarded((n, ht, wd, 2), torch.float32)
    frontend.update_heads(c["dev"]["net"], c["params"], out=(delta, weight))
    assert _guard_ok(dwhole) and _guard_ok(wwhole)
    rd, rw = _ratio(delta, h["delta"], h["d_delta"]), _ratio(weight, h["weight"], h["d_weight"])
    print(f"\nupdate_heads {shape}: worst GPU error / bound: delta {rd:.4f}, weight {rw:.4f}")
    assert rd <= 1.0 and rw <= 1.0
    assert ((weight > 0) & (weight < 1)).all()
    # the reference's call form (a leading batch dimension, the state_dict itself); two runs are bit-identical
    d2, w2 = frontend.update_heads(c["dev"]["net"][None], c["sd"])
    assert d2.shape == (n, ht, wd, 2) and d2.dtype == torch.float32
    assert torch.equal(d2, delta) and torch.equal(w2, weight)


@pytest.mark.parametrize("shape", SHAPES + [(9, 3, 5)], ids=_ids)
def test_graph_agg_against_oracle(shape):
    from wgsr import frontend
    c = _case(shape)
    n, ht, wd = shape
    G, a = c["G"], c["agg"]
    (eta, ewhole), (feat, fwhole) = _guarded((G, ht, wd), torch.float32), _guarded((G, 128, ht, wd), torch.float16)
    frontend.graph_agg(c["dev"]["net"], c["dev"]["ii"], c["params"], out=(eta, feat))
    assert _guard_ok(ewhole) and _guard_ok(fwhole)
    re, rf = _ratio(eta, a["eta"], a["d_eta"]), _ratio(feat, a["feat"], a["d_feat"])
    print(f"\ngraph_agg {shape} ii={c['ii'].tolist()}: worst GPU error / bound: eta {re:.4f}, feat {rf:.4f}")
    assert re <= 1.0 and rf <= 1.0 and (eta > 0).all()
    # the groups given by the caller (no host read), the batch dimension, the state_dict: the same bits
    e2, f2 = frontend.graph_agg(c["dev"]["net"][None], None, c["sd"], ix=c["dev"]["ix"], num_groups=G)
    assert e2.shape == (G, ht, wd) and f2.shape == (G, 128, ht, wd) and f2.dtype == torch.float16
    assert torch.equal(e2, eta) and torch.equal(f2, feat)


def test_graph_agg_with_an_empty_group():
    """caller-given ix = [0, 2, 0] of 4 groups: groups 1 and 3 have no edge and a zero mean (scatter_mean)"""
    from wgsr import frontend
    c = _case(SHAPES[0])
    n, ht, wd = SHAPES[0]
    ix, G = np.array([0, 2, 0]), 4
    a = hr.graph_agg(c["net"], ix, G, c["P"])
    assert not a["mean"][1].any() and not a["mean"][3].any() and a["mean"][2].any()
    eta, feat = frontend.graph_agg(c["dev"]["net"], None, c["params"], ix=torch.from_numpy(ix).cuda(), num_groups=G)
    re, rf = _ratio(eta, a["eta"], a["d_eta"]), _ratio(feat, a["feat"], a["d_feat"])
    print(f"\ngraph_agg with empty groups: worst GPU error / bound: eta {re:.4f}, feat {rf:.4f}")
    assert re <= 1.0 and rf <= 1.0
    assert torch.equal(feat[1], feat[3]) and torch.equal(eta[1], eta[3])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_recorded_reference_outputs(tag):
    """the reference's own modules, run in float64 without any rounding point: within d + r"""
    from wgsr import frontend
    c = hr.fixture_case(tag)
    z, P = c["z"], c["P"]
    h, a = hr.heads(c["net"], P), hr.graph_agg(c["net"], c["ix"], c["G"], P)
    net = torch.from_numpy(c["net"]).cuda()
    sd = _state_dict(P)
    delta, weight = frontend.update_heads(net, sd)
    eta, feat = frontend.graph_agg(net, torch.from_numpy(z[f"{tag}_ii"]).cuda(), sd)
    worst = {}
    for name, got, o in (("delta", delta, h), ("weight", weight, h), ("eta", eta, a), ("feat", feat, a)):
        worst[name] = _ratio(got, z[f"{tag}_{name}"], o["d_" + name] + o["r_" + name])
    print(f"\nfixture {tag}: worst GPU error / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_feat_feeds_upsample_from_features_unchanged():
    """graph_agg's feat and an identical float16 tensor made by torch give the same disps_up, bit for bit"""
    from wgsr import frontend
    c = _case(SHAPES[1])
    n, ht, wd = SHAPES[1]
    G = c["G"]
    eta, feat = frontend.graph_agg(c["dev"]["net"], c["dev"]["ii"], c["params"])
    copy = torch.from_numpy(feat.cpu().numpy().copy()).cuda()
    g = torch.Generator(device="cuda").manual_seed(5)
    disps = 0.1 + torch.rand(G + 2, ht, wd, device="cuda", generator=g)
    w = (3.0 / 128 ** 0.5 * torch.randn(576, 128, device="cuda", generator=g)).half()
    b = 0.5 * torch.randn(576, device="cuda", generator=g)
    kx = torch.tensor([G + 1, 0][:G] if G <= 2 else list(range(G)), device="cuda")
    up1 = torch.full((G + 2, 8 * ht, 8 * wd), FILL, device="cuda")
    up2 = up1.clone()
    frontend.upsample_from_features(disps, up1, kx, feat, w, b)
    frontend.upsample_from_features(disps, up2, kx, copy, w, b)
    assert torch.equal(up1, up2) and (up1[kx] > 0).all()


def test_zero_weights_give_the_activation_of_the_bias_everywhere():
    """border pixels included: a halo that is not zeroed (or any stray term) shows"""
    from wgsr import frontend
    n, ht, wd = 2, 9, 19
    rng = np.random.default_rng(9)
    net = torch.from_numpy(rng.standard_normal((n, 128, ht, wd)).astype(np.float16)).cuda()
    P = hr.make_params(rng)
    P = {k: (np.zeros_like(w), b) for k, (w, b) in P.items()}
    sd = _state_dict(P)
    hidden = frontend.conv3x3_relu(net, frontend.pack_conv3x3(sd["update.delta.0.weight"], sd["update.delta.0.bias"]))
    want = torch.relu(sd["update.delta.0.bias"]).half()
    assert (want > 0).any() and (want == 0).any()
    assert torch.equal(hidden, want.view(1, 128, 1, 1).expand(n, 128, ht, wd))
    delta, weight = frontend.update_heads(net, sd)
    assert torch.equal(delta, sd["update.delta.2.bias"].view(1, 1, 1, 2).expand(n, ht, wd, 2))
    eta, feat = frontend.graph_agg(net, torch.tensor([1, 0], device="cuda"), sd)
    assert torch.equal(feat, torch.relu(sd["update.agg.conv2.bias"]).half().view(1, 128, 1, 1).expand(2, 128, ht, wd))
    # sigmoid and softplus are evaluated in fp32 on the device: the same bits at every pixel, within the
    # oracle's term for the evaluation (8 x 2^-24 of the value) of the float64 function of the bias
    for got, ref in ((weight, hr.sigmoid(P["weight.2"][1].astype(np.float64)).reshape(1, 1, 1, 2)),
                     (eta, 0.01 * hr.softplus(P["agg.eta.0"][1].astype(np.float64)).reshape(1, 1, 1))):
        assert torch.equal(got, got[:1, :1, :1].expand_as(got))
        assert _ratio(got, np.broadcast_to(ref, got.shape), 8 * hr.U32 * ref) <= 1.0


def test_one_hot_weights_reproduce_the_shifted_input_channel():
    """tap and channel ordering and the packed layout: W[o, c, ky, kx] = 1 alone in row o gives
    out[o, y, x] = ReLU(in[c, y + ky - 1, x + kx - 1]) exactly, zero where that lies outside the map"""
    from wgsr import frontend
    n, ht, wd = 2, 9, 19
    rng = np.random.default_rng(19)
    net = torch.from_numpy(rng.standard_normal((n, 128, ht, wd)).astype(np.float16)).cuda()
    pad = torch.nn.functional.pad(torch.relu(net), (1, 1, 1, 1))
    w = torch.zeros(128, 128, 3, 3, dtype=torch.float16, device="cuda")
    rows = {}
    for i in range(36):  # every tap four times, distinct output rows, channels from every K-step and lane group
        o, ch, tap = (11 * i + 3) % 128, (37 * i + 5) % 128, i % 9
        w[o, ch, tap // 3, tap % 3] = 1.0
        rows[o] = (ch, tap)
    zero = torch.zeros(128, device="cuda")
    out = frontend.conv3x3_relu(net, frontend.pack_conv3x3(w, zero))
    for o in range(128):
        if o in rows:
            ch, tap = rows[o]
            want = pad[:, ch, tap // 3:tap // 3 + ht, tap % 3:tap % 3 + wd]
            assert torch.equal(out[:, o], want), (o, ch, tap)
        else:
            assert not out[:, o].any(), o
    # the fp32 heads: hidden row o = ReLU(net[ch]) (centre tap), delta.2 row k reads hidden channel o at a tap
    for tap in range(9):
        sd = _state_dict({k: (np.zeros_like(wt), np.zeros_like(b)) for k, (wt, b) in hr.make_params(rng).items()})
        o, ch = (13 * tap + 7) % 128, (29 * tap + 70) % 128
        sd["update.delta.0.weight"][o, ch, 1, 1] = 1.0
        sd["update.delta.2.weight"][1, o, tap // 3, tap % 3] = 1.0
        delta, weight = frontend.update_heads(net, sd)
        want = pad[:, ch, tap // 3:tap // 3 + ht, tap % 3:tap % 3 + wd].float()
        assert torch.equal(delta[..., 1], want) and not delta[..., 0].any(), tap
        assert torch.equal(weight, torch.full_like(weight, 0.5))


def test_group_sums_do_not_depend_on_the_rest_of_the_graph():
    """a group's feat is the same bits whether its edges are the whole call or lie among other groups'
    (more workgroups, other edge indices), and with every CU busy: 24 edges of 48 x 64"""
    from wgsr import frontend
    c = _case(SHAPES[3])
    net2 = c["dev"]["net"]                                     # 2 x 128 x 48 x 64
    alone_eta, alone_feat = frontend.graph_agg(net2, None, c["params"], ix=torch.tensor([0, 0], device="cuda"),
                                               num_groups=1)
    net = net2.repeat(12, 1, 1, 1)                             # edges 2 k and 2 k + 1 are copies of the two
    ix = torch.arange(24, device="cuda") // 2                  # group k = the same pair
    eta, feat = frontend.graph_agg(net, None, c["params"], ix=ix, num_groups=12)
    for k in range(12):
        assert torch.equal(feat[k], alone_feat[0]) and torch.equal(eta[k], alone_eta[0]), k
    # the same pair as edges 5 and 16 of a graph whose other edges belong to other groups
    ix = torch.full((24,), 1, device="cuda")
    ix[5] = ix[16] = 0
    mixed = net.clone()
    mixed[5], mixed[16] = net2[0], net2[1]
    e3, f3 = frontend.graph_agg(mixed, None, c["params"], ix=ix, num_groups=2)
    assert torch.equal(f3[0], alone_feat[0]) and torch.equal(e3[0], alone_eta[0])
    # update_heads with every CU busy: each copy gives the bits of the two-edge call checked against the oracle
    d2, w2 = frontend.update_heads(net2, c["params"])
    d24, w24 = frontend.update_heads(net, c["params"])
    assert torch.equal(d24.view(12, 2, 48, 64, 2), d2[None].expand(12, 2, 48, 64, 2))
    assert torch.equal(w24.view(12, 2, 48, 64, 2), w2[None].expand(12, 2, 48, 64, 2))


def test_unchecked_calls_replay_from_a_graph_to_the_same_bits():
    from wgsr import frontend
    c = _case(SHAPES[2])
    n, ht, wd = SHAPES[2]
    d, G, p = c["dev"], c["G"], c["params"]
    delta, weight = frontend.update_heads(d["net"], p)
    eta, feat = frontend.graph_agg(d["net"], None, p, ix=d["ix"], num_groups=G)
    again = frontend.graph_agg(d["net"], None, p, ix=d["ix"], num_groups=G)
    assert torch.equal(again[0], eta) and torch.equal(again[1], feat)   # two runs are bit-identical
    torch.cuda.synchronize()
    bufs = [torch.full_like(t, FILL) for t in (delta, weight, eta, feat)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frontend.update_heads(d["net"], p, out=(bufs[0], bufs[1]))
        frontend.graph_agg(d["net"], None, p, ix=d["ix"], num_groups=G, check=False, out=(bufs[2], bufs[3]))
    for t in bufs:
        t.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(bufs, (delta, weight, eta, feat)):
        assert torch.equal(got, want)


def test_out_of_range_ix_raises_and_writes_nothing():
    from wgsr import frontend
    c = _case(SHAPES[2])
    n, ht, wd = SHAPES[2]
    d, G, p = c["dev"], c["G"], c["params"]
    for bad_value in (G, -1):
        bad = d["ix"].clone()
        bad[3] = bad_value
        (eta, ewhole), (feat, fwhole) = _guarded((G, ht, wd), torch.float32), _guarded((G, 128, ht, wd), torch.float16)
        with pytest.raises(RuntimeError, match="outside"):
            frontend.graph_agg(d["net"], None, p, ix=bad, num_groups=G, out=(eta, feat))
        assert (ewhole == FILL).all() and (fwhole == FILL).all()
        # unchecked: no exception, and still nothing written
        frontend.graph_agg(d["net"], None, p, ix=bad, num_groups=G, check=False, out=(eta, feat))
        torch.cuda.synchronize()
        assert (ewhole == FILL).all() and (fwhole == FILL).all()


def test_argument_errors():
    from wgsr import frontend
    c = _case(SHAPES[0])
    d, p = c["dev"], c["params"]
    with pytest.raises(NotImplementedError, match="autocast"):
        frontend.update_heads(d["net"].float(), p)
    with pytest.raises(NotImplementedError, match="autocast"):
        frontend.graph_agg(d["net"].float(), d["ii"], p)
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.update_heads(d["net"].cpu(), p)
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.graph_agg(d["net"].cpu(), d["ii"], p)
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="net requires grad"):
            frontend.update_heads(d["net"].clone().requires_grad_(), p)
    with pytest.raises(ValueError, match="net must be"):
        frontend.update_heads(d["net"][:, :64].contiguous(), p)
    with pytest.raises(ValueError, match="together"):
        frontend.graph_agg(d["net"], d["ii"], p, ix=d["ix"])
    with pytest.raises(ValueError, match="group indices"):
        frontend.graph_agg(d["net"], d["ii"][:2], p)
    with pytest.raises(ValueError, match="packed pair"):
        frontend.conv3x3_relu(d["net"], (p.hidden[0][:-8], p.hidden[1]))
    with pytest.raises(RuntimeError, match="multiple of 128"):
        frontend.conv3x3_relu(d["net"], p.delta)
    # no edges: nothing to do
    delta, weight = frontend.update_heads(d["net"][:0], p)
    assert delta.shape == (0, 3, 5, 2) and weight.shape == (0, 3, 5, 2)
    # no edges but two groups: both empty, the mean zero, feat = ReLU(conv2's bias) everywhere
    eta, feat = frontend.graph_agg(d["net"][:0], None, p, ix=d["ix"][:0], num_groups=2)
    want = torch.relu(c["sd"]["update.agg.conv2.bias"]).half().view(1, 128, 1, 1).expand(2, 128, 3, 5)
    assert torch.equal(feat, want) and eta.shape == (2, 3, 5) and torch.isfinite(eta).all()
