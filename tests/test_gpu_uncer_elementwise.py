"""GPU: the uncertainty mapping loss (unc_fwd, unc_small, unc_loss, unc_bwd
and the SSIM kernels under them, through wgsr.uncertainty.loss_forward /
loss_backward) against the float64 oracle, pixel by pixel
(tests/_loss_elementwise_ref.py holds the cases, the exclusion of pixels
whose decisions sit at their thresholds and the bound;
tests/test_loss_elementwise_ref.py shows on the CPU that the check fails on
one halved d_image pixel, one d_unc entry taken from its neighbour and a
one-pixel shift of the small map's resampling grid).

Checked: d_image and d_depth per pixel, d_unc and the uncertainty loss per
feature-resolution pixel, the loss and both exposure gradients.  Each check
prints its worst err / bound per tensor and per magnitude group (DESIGN.md
records them).
"""
import pytest
import torch

import _loss_elementwise_ref as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def run(c):
    from wgsr.uncertainty import flatten_config, loss_backward, loss_forward
    t = {k: v.to(DEV) for k, v in c.t.items()}
    loss, state = loss_forward(t["ren"], t["dep"], t["opa"], t["gt"], t["ref"], t["ea"], t["eb"], t["unc"], c.tf, c.sf,
                               flatten_config(E.ou.DEFAULT_CONFIG), initialization=c.init)
    d_image, d_depth, d_a, d_b, d_unc = loss_backward(state)
    torch.cuda.synchronize()
    np_ = lambda x: x.detach().cpu().numpy()  # noqa: E731
    return dict(loss=np_(loss), d_image=np_(d_image), d_depth=np_(d_depth), d_unc=np_(d_unc),
                uncertainty_loss=np_(state.uncertainty_loss), d_exposure_a=np_(d_a), d_exposure_b=np_(d_b))


@pytest.mark.parametrize("name", list(E.UNC_CASES))
def test_pixels_match_the_float64_oracle(name):
    c = E.unc_case(name)
    got = run(c)
    if c.init:  # no exposure term: the gradient is absent in the oracle and zero here
        assert not got["d_exposure_a"].any() and not got["d_exposure_b"].any()
    E.unc_check(c, got)
