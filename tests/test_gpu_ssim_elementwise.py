"""GPU: k_ssim_fwd and k_ssim_bwd against the float64 oracle, pixel by pixel
(tests/_loss_elementwise_ref.py holds the cases and the bound;
tests/test_loss_elementwise_ref.py shows on the CPU that the check fails on
a scaled seam column or row, a halved pixel, a wrong plane_scale index and a
dropped halo tap).

Checked per pixel: the three derivative maps the forward keeps (dS/dmu1,
dS/dE[x^2], dS/dE[xy]; through wgsr_ssim_forward), dL/dimg1 (through
wgsr.loss.ssim) and the per-plane means.  Each check prints its worst
err / bound per tensor and per variance group (DESIGN.md records them).
"""
import pytest
import torch

import _loss_elementwise_ref as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def run(c):
    from wgsr import _lib
    from wgsr.loss import ssim
    L = _lib.load()
    ren, gt = c.ren.to(DEV), c.gt.to(DEV)
    H, W = c.shape[-2:]
    planes = ren.numel() // (H * W)
    nan = float("nan")
    dmap = torch.full((3 * planes * H * W,), nan, device=DEV)
    plane_mean = torch.full((planes,), nan, device=DEV)
    mean = torch.full((), nan, device=DEV)
    with torch.cuda.device(DEV), _lib.AllocRequest(DEV):
        _lib.check(L.wgsr_ssim_forward(ren.data_ptr(), gt.data_ptr(), planes, H, W, c.ws, dmap.data_ptr(),
                                       plane_mean.data_ptr(), mean.data_ptr(), _lib.ALLOC_SCRATCH, None,
                                       _lib.stream_handle(DEV)))
    x = ren.clone().requires_grad_(True)
    val = ssim(x, gt, c.ws, size_average=c.weights is None)
    E.ssim_loss(val, c.weights).backward()
    d = dmap.view(3, planes, H, W).cpu().numpy()
    return dict(grad=x.grad.view(planes, H, W).cpu().numpy(), dmap0=d[0], dmap1=d[1], dmap2=d[2],
                plane_mean=plane_mean.cpu().numpy())


@pytest.mark.parametrize("name", E.ssim_case_names())
def test_pixels_match_the_float64_oracle(name):
    c = E.ssim_case(name)
    E.ssim_check(c, run(c))
