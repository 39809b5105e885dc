"""What the mapper reads from the tracker's ``DepthVideo``, over the
``droid_backends`` kernels (csrc/droid.hip) and without ``lietorch``:

* ``distance``          DepthVideo.distance (depth_video.py:205-235)
* ``valid_depth_mask``  DepthVideo.update_valid_depth_mask (depth_video.py:407-442)
* ``depth_and_pose``    the non-metric branch of DepthVideo.get_depth_and_pose
                        with get_w2c_and_depth's validity flag (mapper.py:574-599)
* ``ba``                DepthVideo.ba (depth_video.py:351-373): the dense bundle
                        adjustment (csrc/droid_ba.hip)

poses [num, 7] = (tx, ty, tz, qx, qy, qz, qw), world to camera; disps
[num, ht, wd]; intrinsics [4] = (fx, fy, cx, cy); device fp32 tensors.
"""
from __future__ import annotations

import torch

import droid_backends

MIN_VALID_DEPTHS = 100  # mapper.py:593


def distance(poses, disps, intrinsics, ii=None, jj=None, beta=0.3, bidirectional=True):
    """The frame distance of pairs (ii[k], jj[k]); with ``ii`` None the N x N
    matrix over all ``poses.shape[0]`` frames.  The bidirectional form is one
    fused launch (the reference makes two and averages)."""
    matrix = ii is None
    dev = poses.device
    if matrix:
        N = poses.shape[0]
        ii, jj = torch.meshgrid(torch.arange(N, device=dev), torch.arange(N, device=dev), indexing="ij")
    ii = torch.as_tensor(ii).to(dev, torch.int64).reshape(-1).contiguous()
    jj = torch.as_tensor(jj).to(dev, torch.int64).reshape(-1).contiguous()
    d = droid_backends.frame_distance(poses.contiguous(), disps.contiguous(), intrinsics.contiguous(), ii, jj, beta,
                                      bidirectional=bidirectional)
    return d.reshape(N, N) if matrix else d


@torch.no_grad()
def valid_depth_mask(poses, disps, intrinsics, index, thresh=0.01, visible_num=2):
    """masks [m, ht, wd] (bool) of frames ``index``: a pixel is valid when at
    least ``visible_num`` neighbour frames agree with its depth to within
    ``thresh`` x the frame's mean depth, and its depth is under 3 x the
    median of the frame's agreeing depths.  A frame with no agreeing pixel
    gets an all-False mask (its median is NaN)."""
    index = torch.as_tensor(index).to(poses.device, torch.int64).reshape(-1).contiguous()
    depths = 1.0 / torch.index_select(disps, 0, index)
    th = (thresh * depths.mean(dim=[1, 2])).contiguous()
    count = droid_backends.depth_filter(poses.contiguous(), disps.contiguous(), intrinsics.contiguous(), index, th)
    depths[~(count >= visible_num)] = torch.nan
    median = depths.view(depths.shape[0], -1).nanmedian(dim=1).values
    return depths < 3 * median[:, None, None]


def pose_to_c2w(pose7):
    """The 4 x 4 camera-to-world matrix of one (tx, ty, tz, qx, qy, qz, qw)
    world-to-camera pose: the inverse [R^T | -R^T t]."""
    p = pose7.to(torch.float32)
    t, (x, y, z, w) = p[:3], p[3:]
    R = torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)]),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)]),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])])
    c2w = torch.eye(4, dtype=torch.float32, device=p.device)
    c2w[:3, :3] = R.T
    c2w[:3, 3] = -(R.T @ t)
    return c2w


@torch.no_grad()
def depth_and_pose(pose7, disp, mask):
    """(depth [ht, wd], mask, c2w [4, 4], invalid) of one frame: depth =
    1 / disp, c2w the inverse of the quaternion pose, invalid = fewer than 100
    valid depths.  ``OnlineMapper.update_keyframes`` takes
    ``{uid: (torch.linalg.inv(c2w), depth[None], invalid)}``."""
    depth = 1.0 / disp
    mask = mask.clone()
    invalid = bool(mask.sum() < MIN_VALID_DEPTHS)
    return depth, mask, pose_to_c2w(pose7), invalid


@torch.no_grad()
def ba(poses, disps, intrinsics, target, weight, eta, ii, jj, t0=1, t1=None, iters=2, lm=1e-4, ep=0.1,
       motion_only=False, uncertainties_inv=None, mono_disps=None, mono_valid_mask=None):
    """DepthVideo.ba on the buffers themselves: ``poses`` and ``disps`` are
    updated in place and the disparities clamped to >= 1e-5.  ``target`` and
    ``weight`` are the update operator's [1, N, ht, wd, 2]; with
    ``uncertainties_inv`` [num, ht, wd] the weight of edge e is multiplied by
    that of its source frame; ``mono_disps`` masked by ``mono_valid_mask``
    (both [num, ht, wd]) are the sensor disparities, else there are none.
    ``t1`` None: max(ii, jj) + 1, the one host read."""
    ht, wd = disps.shape[1], disps.shape[2]
    if uncertainties_inv is not None:
        weight = weight * uncertainties_inv[ii][None, :, :, :, None]
    target = target.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    weight = weight.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    if mono_disps is not None and mono_valid_mask is not None:
        disps_sens = (mono_disps * mono_valid_mask).contiguous()
    else:
        disps_sens = torch.zeros_like(disps)
    if t1 is None:
        t1 = int(max(ii.max().item(), jj.max().item())) + 1
    out = droid_backends.ba(poses, disps, intrinsics, disps_sens, target, weight, eta, ii, jj, t0, t1, iters, lm, ep,
                            motion_only, False)
    disps.clamp_(min=1e-5)
    return out
