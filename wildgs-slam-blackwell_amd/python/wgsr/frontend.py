"""What the mapper reads from the tracker's ``DepthVideo``, over the
``droid_backends`` kernels (csrc/droid.hip) and without ``lietorch``:

* ``distance``          DepthVideo.distance (depth_video.py:205-235)
* ``valid_depth_mask``  DepthVideo.update_valid_depth_mask (depth_video.py:407-442)
* ``depth_and_pose``    the non-metric branch of DepthVideo.get_depth_and_pose
                        with get_w2c_and_depth's validity flag (mapper.py:574-599)

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
