"""GPU: the uncertainty MLP's forward and backward kernels against the
float64 oracle, row by row and parameter element by parameter element
(tests/_loss_elementwise_ref.py holds the cases, the near-row masking and the
bound; tests/test_loss_elementwise_ref.py shows on the CPU that the check
fails on one scaled row of u, one scaled 64-column chunk of dW1 and one
dropped row).

The kernel paths are selected by shape and alignment alone (MLP_CASES names
the kernels each case reaches): k_mlp_fwd_small<64 / 256 / 384>,
k_mlp_fwd<16> at C = 192 and at a 4-byte offset, k_mlp_fwd<64> and k_mlp_bwd
at 1025 row blocks with 65 reduce segments, k_mlp_bwd2, the two-segment
launches and the accumulating backward.  Each check prints its worst
err / bound per tensor and per magnitude group (DESIGN.md records them).
"""
import numpy as np
import pytest
import torch

import _loss_elementwise_ref as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _net(c):
    from wgsr.mlp import UncertaintyMLP
    net = UncertaintyMLP(input_dim=c.C, dropout_p=c.p).to(DEV)
    with torch.no_grad():
        for prm, w in zip(net.parameters(), c.weights):
            prm.copy_(w.to(DEV))
    return net


def _features(c):
    """The case's rows on the device: 16-byte aligned, or the same rows at a
    4-byte offset (which takes the VALU kernels)."""
    if not c.misaligned:
        x = c.x.to(DEV)
    else:
        x = torch.empty(c.N * c.C + 1, device=DEV)[1:].view(c.N, c.C)
        x.copy_(c.x)
    assert (x.data_ptr() % 16 != 0) == c.misaligned
    return x


def _seed_dev(seed):
    return torch.tensor([seed], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("name", list(E.MLP_CASES))
def test_rows_and_gradients_match_the_float64_oracle(name):
    c = E.mlp_case(name)
    net = _net(c)
    net.seed_source = lambda: c.seed
    u = net(_features(c).view(1, c.N, c.C))
    (u.view(-1) * c.du.to(DEV)).sum().backward()
    got = {k: prm.grad.cpu().numpy() for k, prm in zip(E.MLP_PARAMS, net.parameters())}
    got["u"] = u.detach().view(-1).cpu().numpy()
    E.mlp_check(c, got)


def _seg2_inputs():
    c = E.mlp_seg2_case()
    net = _net(c.a)
    x1, x2 = c.a.x.to(DEV), c.b.x.to(DEV)
    return c, net, x1, x2, c.a.du.to(DEV), c.b.du.to(DEV), _seed_dev(c.a.seed), _seed_dev(c.b.seed)


def test_two_segments_match_the_two_single_runs_summed():
    """forward_raw2 / backward_raw2 (one launch over both row segments, each
    with its own seed and scale) against the float64 sum of the two
    single-segment runs."""
    from wgsr import mlp
    c, net, x1, x2, du1, du2, s1, s2 = _seg2_inputs()
    u, saved = mlp.forward_raw2(net, x1, x2, s1, s2)
    flat = mlp.backward_raw2(saved, du1, du2, *c.scales)
    got = E.mlp_split_grad(flat.cpu().numpy(), c.a.C)
    got["u"] = u.cpu().numpy()
    E.mlp_check(c, got)


def test_accumulated_backward_matches_the_float64_sum():
    """backward_raw with ``accumulate_into``: the second segment's backward
    added in place to the first one's gradient."""
    from wgsr import mlp
    c, net, x1, x2, du1, du2, s1, s2 = _seg2_inputs()
    u1, saved1 = mlp.forward_raw(net, x1, s1)
    u2, saved2 = mlp.forward_raw(net, x2, s2)
    flat = mlp.backward_raw(saved1, du1, c.scales[0])
    out = mlp.backward_raw(saved2, du2, c.scales[1], accumulate_into=flat)
    assert out.data_ptr() == flat.data_ptr()
    got = E.mlp_split_grad(flat.cpu().numpy(), c.a.C)
    got["u"] = np.concatenate([u1.cpu().numpy(), u2.cpu().numpy()])
    E.mlp_check(c, got)
