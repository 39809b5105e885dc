"""GPU: csrc/tracking.hip element by element against the float64 oracle
(tests/_map_elementwise_ref.py holds the cases, the decisions and the bound;
tests/test_map_elementwise_ref.py shows on the CPU that the checks fail on a
halved d_image pixel, a d_opacity pixel taken from its neighbour, a dropped
last workgroup, the upper median, a block left at 1 under 1 <= t, replicate
padding of the top row, Vm with c2 and c3 swapped, an unsigned camera centre
and a second moment without its bias correction).

* k_track_loss through wgsr.tracking.tracking_loss: d_image and d_opacity per
  pixel, the loss and both exposure gradients; four shapes x (grad mask,
  uncertainty) on and off.
* k_grad_intensity and k_grad_block through wgsr.tracking.compute_grad_mask:
  the raw intensity per pixel inside the bound where no block touches it; the
  block pixels EXACTLY off the flagged ones.
* k_pose_step through wgsr_pose_step on a guarded state: all 68 floats after
  one step, the converged flag, and camera_only.

Each check prints its worst err / bound per tensor (DESIGN.md records them).
"""
import numpy as np
import pytest
import torch

import _map_elementwise_ref as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _np(x):
    return x.detach().cpu().numpy()


@pytest.mark.parametrize("name", E.track_case_names())
def test_track_loss_pixels_match_the_float64_oracle(name):
    from wgsr.tracking import tracking_loss
    c = E.track_case(name)
    t = {k: v.to(DEV) for k, v in c.t.items()}
    r, o, a, b = (t[k].clone().requires_grad_(True) for k in ("ren", "opa", "ea", "eb"))
    loss = tracking_loss(r, o, t["gt"], a, b, t["gm"] if c.use_gm else None, t["unc"] if c.use_unc else None,
                         E.RGB_TH)
    loss.backward()
    torch.cuda.synchronize()
    E.track_check(c, dict(loss=_np(loss), d_image=_np(r.grad), d_opacity=_np(o.grad), d_exposure_a=_np(a.grad),
                          d_exposure_b=_np(b.grad)))


@pytest.mark.parametrize("name", list(E.GMASK_CASES))
def test_grad_mask_pixels_match_the_float64_oracle(name):
    from wgsr.tracking import compute_grad_mask
    c = E.gmask_case(name)
    got = compute_grad_mask(torch.from_numpy(c.img).to(DEV), c.mult)
    torch.cuda.synchronize()
    assert got.shape == (1, c.H, c.W)
    E.gmask_check(c, _np(got)[0])


def _pose_step(c, camera_only):
    from wgsr import _lib
    L = _lib.load()
    assert int(L.wgsr_pose_state_floats()) == 68
    st = E.Guarded((68,), init=c.st)
    conv = E.Guarded((1,), dtype=torch.int32)
    dtau, part, proj = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (c.dtau, c.part, c.proj))
    b1, b2 = E.POSE_BETAS
    with torch.cuda.device(DEV):
        if camera_only:
            _lib.check(L.wgsr_pose_step(st.ptr(), None, None, 0, _lib.ptr(proj), 0.0, 0.0, 0.0, b1, b2, E.POSE_EPS, 0,
                                        0.0, None, 1, _lib.stream_handle(DEV)))
        else:
            _lib.check(L.wgsr_pose_step(st.ptr(), _lib.ptr(dtau), _lib.ptr(part), c.n_part, _lib.ptr(proj), c.lr[0],
                                        c.lr[1], c.lr[2], b1, b2, E.POSE_EPS, c.step, E.POSE_CONV_TH, conv.ptr(), 0,
                                        _lib.stream_handle(DEV)))
    torch.cuda.synchronize()
    return st.read(written=False), conv.read(written=not camera_only)


@pytest.mark.parametrize("name", E.pose_case_names())
def test_pose_step_state_matches_the_float64_oracle(name):
    c = E.pose_case(name)
    got, conv = _pose_step(c, camera_only=False)
    assert not (got[32:68] == np.float32(7.0)).any()   # every camera field and |tau| rewritten
    E.pose_check(c, got, int(conv[0]))


@pytest.mark.parametrize("name", ["a0.01_s7_n3", "a1_s1_n1500"])
def test_pose_step_camera_only_keeps_the_state(name):
    c = E.pose_case(name)
    got, _ = _pose_step(c, camera_only=True)
    E.pose_check_camera(c, got)
