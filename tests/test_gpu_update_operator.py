"""GPU tests of the whole update operator as one call
(wgsr.frontend.update_operator / UpdateOperator): bit-identity with the
composition of the individual calls (corr_encoder, flow_encoder, conv_gru,
update_heads, graph_agg), each of which has its own tests against its float64
oracle (the wiring of the composition is pinned on the CPU against the recorded
``UpdateModule.forward`` of the reference, tests/test_encoders_ref.py); the call
forms, a graph replay and the status errors.
"""
import numpy as np
import pytest
import torch

import _encoders_ref as er
import _gru_ref as gr
import _update_heads_ref as hr

pytestmark = pytest.mark.gpu

FILL = -7.0
GUARD = 64
SHAPE = (3, 9, 17)      # partial tiles both ways
FRAMES = 4
_cache = {}


def _state_dict(Pe, Pg, Ph, prefix="update."):
    sd = {}
    for name, (w, b) in {**Pe, **{"gru." + k: v for k, v in Pg.items()}, **Ph}.items():
        sd[f"{prefix}{name}.weight"] = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        sd[f"{prefix}{name}.bias"] = torch.from_numpy(np.ascontiguousarray(b)).cuda()
    return sd


def _case():
    """parameters and inputs at SHAPE, computed once and shared (never modified)"""
    if not _cache:
        from wgsr import frontend
        n, ht, wd = SHAPE
        rng = np.random.default_rng(321)
        Pe, Pg, Ph = er.make_params(rng), gr.make_params(rng), hr.make_params(rng)
        sd = _state_dict(Pe, Pg, Ph)
        net, inp = (torch.from_numpy(rng.standard_normal((n, 128, ht, wd)).astype(np.float16)).cuda() for _ in range(2))
        corr, flow = (torch.from_numpy(t).cuda() for t in er.make_inputs(rng, n, ht, wd, round_flow=False))
        inps = torch.from_numpy(rng.standard_normal((FRAMES, 128, ht, wd)).astype(np.float16)).cuda()
        _cache.update(sd=sd, params=frontend.UpdateOperator.from_state_dict(sd), net=net, inp=inp, corr=corr,
                      flow=flow, inps=inps, ii=torch.tensor([2, 0, 2], device="cuda"))
    return _cache


def _composition(c, inp, flow, ii=None, inp_ix=None):
    from wgsr import frontend
    p = c["params"]
    ce = frontend.corr_encoder(c["corr"], p.encoders)
    fe = frontend.flow_encoder(flow, p.encoders)
    net = frontend.conv_gru(c["net"], inp, ce, fe, p.gru, inp_ix=inp_ix)
    out = (net,) + frontend.update_heads(net, p.heads)
    return out if ii is None else out + frontend.graph_agg(net, ii, p.heads)


def _same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), k


def test_bit_identity_with_the_composition_of_the_calls():
    from wgsr import frontend
    c = _case()
    n, ht, wd = SHAPE
    p = c["params"]
    want3 = _composition(c, c["inp"], c["flow"])
    want5 = _composition(c, c["inp"], c["flow"], ii=c["ii"])
    got3 = frontend.update_operator(c["net"], c["inp"], c["corr"], c["flow"], params=p)
    got5 = frontend.update_operator(c["net"], c["inp"], c["corr"], c["flow"], c["ii"], params=p)
    _same(got3, want3)
    _same(got5, want5)
    # what conv_gru / update_heads / graph_agg document
    net, delta, weight, eta, feat = got5
    assert net.shape == (n, 128, ht, wd) and net.dtype == torch.float16
    assert delta.shape == weight.shape == (n, ht, wd, 2) and delta.dtype == weight.dtype == torch.float32
    assert eta.shape == (2, ht, wd) and eta.dtype == torch.float32
    assert feat.shape == (2, 128, ht, wd) and feat.dtype == torch.float16
    # the per-frame inp buffer with an index, against the gathered copy
    ix = torch.tensor([3, 0, 3], device="cuda")
    want = _composition(c, c["inps"][ix].contiguous(), c["flow"], ii=c["ii"])
    got = frontend.update_operator(c["net"], c["inps"], c["corr"], c["flow"], c["ii"], params=p, inp_ix=ix)
    _same(got, want)
    assert not torch.equal(got[0], got5[0])
    # the reference's call form: a leading batch dimension and the state_dict itself; groups given
    got = frontend.update_operator(c["net"][None], c["inp"][None], c["corr"][None], c["flow"][None], c["ii"],
                                   params=c["sd"])
    _same(got, want5)
    ix = torch.tensor([1, 0, 1], device="cuda")
    _same(frontend.update_operator(c["net"], c["inp"], c["corr"], c["flow"], ix, params=p, num_groups=2), want5)


def test_flow_none_is_a_flow_of_zeros():
    from wgsr import frontend
    c = _case()
    zeros = torch.zeros_like(c["flow"])
    want = _composition(c, c["inp"], zeros, ii=c["ii"])
    _same(frontend.update_operator(c["net"], c["inp"], c["corr"], None, c["ii"], params=c["params"]), want)
    _same(frontend.update_operator(c["net"], c["inp"], c["corr"], zeros.half(), c["ii"], params=c["params"]), want)
    got = frontend.update_operator(c["net"][None], c["inp"][None], c["corr"][None], params=c["params"])
    _same(got, want[:3])
    assert not torch.equal(want[0], _composition(c, c["inp"], c["flow"])[0])


def test_unchecked_call_replays_from_a_graph_to_the_eager_bits():
    from wgsr import frontend
    c = _case()
    p = c["params"]
    ix = torch.tensor([3, 0, 3], device="cuda")
    groups = torch.tensor([1, 0, 1], device="cuda")
    args = (c["net"], c["inps"], c["corr"], c["flow"], groups)
    kw = dict(params=p, inp_ix=ix, num_groups=2)
    eager = frontend.update_operator(*args, **kw)
    torch.cuda.synchronize()
    bufs = tuple(torch.full_like(t, FILL) for t in eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = frontend.update_operator(*args, check=False, out=bufs, **kw)
    assert all(a is b for a, b in zip(got, bufs))
    for t in bufs:
        t.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    _same(bufs, eager)


def _guarded_outputs(n, ht, wd, G):
    shapes = (((n, 128, ht, wd), torch.float16), ((n, ht, wd, 2), torch.float32), ((n, ht, wd, 2), torch.float32),
              ((G, ht, wd), torch.float32), ((G, 128, ht, wd), torch.float16))
    wholes = [torch.full((int(np.prod(s)) + GUARD,), FILL, dtype=dt, device="cuda") for s, dt in shapes]
    return tuple(w[:-GUARD].view(s) for w, (s, _) in zip(wholes, shapes)), wholes


def test_out_of_range_indices_raise_the_status_errors():
    from wgsr import frontend
    c = _case()
    n, ht, wd = SHAPE
    p = c["params"]
    groups = torch.tensor([1, 0, 1], device="cuda")
    for bad_value in (-1, FRAMES):
        out, wholes = _guarded_outputs(n, ht, wd, 2)
        with pytest.raises(RuntimeError, match="WGSR_GRU_BAD_IX"):
            frontend.update_operator(c["net"], c["inps"], c["corr"], c["flow"], groups, params=p, num_groups=2,
                                     inp_ix=torch.tensor([1, bad_value, 0], device="cuda"), out=out)
        for whole in wholes:      # the GRU wrote nothing and no later call ran
            assert bool((whole == FILL).all())
    for bad_value in (-1, 2):
        out, wholes = _guarded_outputs(n, ht, wd, 2)
        with pytest.raises(RuntimeError, match="WGSR_GRAPH_AGG_BAD_IX"):
            frontend.update_operator(c["net"], c["inp"], c["corr"], c["flow"],
                                     torch.tensor([1, bad_value, 0], device="cuda"), params=p, num_groups=2, out=out)
        for whole in wholes[3:]:  # eta and feat stay at the sentinel; net', delta and weight are those of the call
            assert bool((whole == FILL).all())
        _same(out[:3], _composition(c, c["inp"], c["flow"]))
        for whole in wholes[:3]:
            assert bool((whole[-GUARD:] == FILL).all())


def test_argument_errors():
    from wgsr import frontend
    c = _case()
    p = c["params"]
    with pytest.raises(ValueError, match="params"):
        frontend.update_operator(c["net"], c["inp"], c["corr"], c["flow"])
    with pytest.raises(ValueError, match="corr must hold"):
        frontend.update_operator(c["net"], c["inp"], c["corr"][:2], c["flow"], params=p)
    with pytest.raises(ValueError, match="flow must hold"):
        frontend.update_operator(c["net"], c["inp"], c["corr"], c["flow"][..., :5], params=p)
    with pytest.raises(NotImplementedError, match="autocast"):
        frontend.update_operator(c["net"], c["inp"], c["corr"].float(), c["flow"], params=p)
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.update_operator(c["net"], c["inp"], c["corr"].cpu(), c["flow"], params=p)
    with pytest.raises(ValueError, match="out must hold"):
        frontend.update_operator(c["net"], c["inp"], c["corr"], c["flow"], params=p, out=(c["net"],))
