"""``lietorch`` on MI355X: the part of the Lie-group package the reference's
tracker uses (src/depth_video.py, src/geom/projective_ops.py,
src/trajectory_filler.py, src/motion_filter.py, src/utils/eval_traj.py),
computed by libwgsr.so's gfx950 kernels (csrc/lie.hip, include/wgsr.h
``wgsr_lie_se3``).

Built: ``SE3`` (data [..., 7] = (tx, ty, tz, qx, qy, qz, qw); tangent vectors
[..., 6] = (tau, phi)), ``cat`` and ``stack``.  ``Sim3``, ``SO3`` and ``RxSO3``
exist as classes, so ``from lietorch import SE3, Sim3`` and ``isinstance(G,
Sim3)`` work; constructing one raises ``NotImplementedError`` naming the group.

Construction, indexing, ``Identity``, ``cat``, ``to`` work on any device.  The
group operations are HIP kernels: on host tensors they raise ``RuntimeError``
("expected a HIP device tensor"); there is no CPU fallback.  They are
inference only: an input that requires grad while grad mode is on raises
``NotImplementedError`` (the tracker runs under ``torch.no_grad``).  Only
float32 is built.  Launches go on torch's current stream.
"""
from __future__ import annotations

from .groups import SE3, SO3, RxSO3, Sim3, LieGroup, cat, stack

__all__ = ["SE3", "SO3", "RxSO3", "Sim3", "LieGroup", "cat", "stack"]
