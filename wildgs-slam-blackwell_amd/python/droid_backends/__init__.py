"""``droid_backends`` on MI355X: the native module the reference imports in
``src/depth_video.py`` and ``src/modules/droid_net/corr.py``
(bindings: src/lib/droid.cpp:254-266), computed by libwgsr.so's gfx950
kernels (csrc/droid.hip, include/wgsr.h ``wgsr_droid_*``).

Built: ``frame_distance``, ``depth_filter``, ``iproj``, ``corr_index_forward``,
``corr_index_backward`` -- the reference's argument order and return shapes
(the two lookups return one-element lists).  Not built yet: ``ba``,
``projmap``, ``altcorr_forward``, ``altcorr_backward``; they raise
``NotImplementedError`` naming the op, so a caller sees at once what is
missing.  Launches go on torch's current stream.
"""
from __future__ import annotations

import torch

from wgsr import _lib

__all__ = ["ba", "frame_distance", "projmap", "depth_filter", "iproj", "altcorr_forward", "altcorr_backward",
           "corr_index_forward", "corr_index_backward"]

_DTYPE_TAG = {torch.float32: 0, torch.float16: 1}  # WGSR_DTYPE_F32 / WGSR_DTYPE_F16


def _contiguous(**tensors):
    # the reference's CHECK_CONTIGUOUS(x): "<x> must be contiguous"
    for name, t in tensors.items():
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")


def _device_of(**tensors):
    dev = None
    for name, t in tensors.items():
        if t.device.type != "cuda":
            raise RuntimeError(f"{name}: expected a HIP device tensor, got {t.device}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"{name}: expected a tensor on {dev}, got {t.device}")
    return dev


def _frames(poses, disps, intrinsics):
    if poses.dim() != 2 or poses.size(1) != 7:
        raise RuntimeError("poses must have dimensions (num, 7)")
    if disps.dim() != 3:
        raise RuntimeError("disps must have dimensions (num, ht, wd)")
    if intrinsics.numel() != 4:
        raise RuntimeError("intrinsics must have 4 elements (fx, fy, cx, cy)")
    for name, t in (("poses", poses), ("disps", disps), ("intrinsics", intrinsics)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32")
    # (the reference passes poses[:counter] with the whole disps buffer)
    return min(poses.size(0), disps.size(0)), disps.size(1), disps.size(2)


def _index(name, t):
    if t.dim() != 1 or t.dtype != torch.int64:
        raise RuntimeError(f"{name} must be a 1-D int64 tensor")
    return t


def frame_distance(poses, disps, intrinsics, ii, jj, beta, bidirectional=False):
    """dist [n]: DepthVideo.distance's metric from frame ii[k] to frame jj[k].
    ``bidirectional`` (not in the reference's signature): 0.5 (d(ii, jj) +
    d(jj, ii)) in the same launch."""
    _contiguous(poses=poses, disps=disps, intrinsics=intrinsics, ii=ii, jj=jj)
    dev = _device_of(poses=poses, disps=disps, intrinsics=intrinsics, ii=ii, jj=jj)
    num, ht, wd = _frames(poses, disps, intrinsics)
    _index("ii", ii)
    _index("jj", jj)
    if ii.numel() != jj.numel():
        raise RuntimeError("ii and jj must have the same length")
    n = ii.numel()
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return dist
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_frame_distance(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), num, ht, wd,
                                               ii.data_ptr(), jj.data_ptr(), n, float(beta), int(bool(bidirectional)),
                                               dist.data_ptr(), _lib.stream_handle(dev)))
    return dist


def depth_filter(poses, disps, intrinsics, ix, thresh):
    """count [m, ht, wd] (fp32): the multi-view consistency count of frames
    ix[b] against their neighbours ix-1, ix-2, ix-3, ix+3, ix+4, ix+5."""
    _contiguous(poses=poses, disps=disps, intrinsics=intrinsics, ix=ix, thresh=thresh)
    dev = _device_of(poses=poses, disps=disps, intrinsics=intrinsics, ix=ix, thresh=thresh)
    num, ht, wd = _frames(poses, disps, intrinsics)
    _index("ix", ix)
    if thresh.dim() != 1 or thresh.dtype != torch.float32 or thresh.numel() != ix.numel():
        raise RuntimeError("thresh must be a float32 tensor with one value per index")
    m = ix.numel()
    count = torch.empty(m, ht, wd, dtype=torch.float32, device=dev)
    if m == 0:
        return count
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_depth_filter(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), num, ht, wd,
                                             ix.data_ptr(), thresh.data_ptr(), m, count.data_ptr(),
                                             _lib.stream_handle(dev)))
    return count


def iproj(poses, disps, intrinsics):
    """points [num, ht, wd, 3]: every pixel back-projected, (R(q) X + d t) / d."""
    _contiguous(poses=poses, disps=disps, intrinsics=intrinsics)
    dev = _device_of(poses=poses, disps=disps, intrinsics=intrinsics)
    _, ht, wd = _frames(poses, disps, intrinsics)
    num = disps.size(0)
    if poses.size(0) < num:
        raise RuntimeError("poses must have a row per frame of disps")
    points = torch.empty(num, ht, wd, 3, dtype=torch.float32, device=dev)
    if points.numel() == 0:
        return points
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_iproj(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), num, ht, wd,
                                      points.data_ptr(), _lib.stream_handle(dev)))
    return points


def _lookup_shapes(volume, coords):
    if volume.dim() != 5:
        raise RuntimeError("volume must have dimensions (n, h1, w1, h2, w2)")
    if volume.dtype not in _DTYPE_TAG:
        raise RuntimeError(f"volume must be float32 or float16, got {volume.dtype}")
    n, h1, w1, h2, w2 = volume.shape
    if coords.dtype != torch.float32 or tuple(coords.shape) != (n, 2, h1, w1):
        raise RuntimeError("coords must be a float32 tensor of dimensions (n, 2, h1, w1)")
    return n, h1, w1, h2, w2


def corr_index_forward(volume, coords, radius):
    """[corr [n, 2r+1, 2r+1, h1, w1]]: the bilinear window lookup of
    CorrSampler.forward; the first window index runs along x."""
    _contiguous(volume=volume, coords=coords)
    dev = _device_of(volume=volume, coords=coords)
    n, h1, w1, h2, w2 = _lookup_shapes(volume, coords)
    r = int(radius)
    corr = torch.empty(n, 2 * r + 1, 2 * r + 1, h1, w1, dtype=volume.dtype, device=dev)
    if corr.numel() == 0:
        return [corr]
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_corr_index_forward(volume.data_ptr(), coords.data_ptr(), _DTYPE_TAG[volume.dtype],
                                                   n, h1, w1, h2, w2, r, corr.data_ptr(), _lib.stream_handle(dev)))
    return [corr]


def corr_index_backward(volume, coords, corr_grad, radius):
    """[volume_grad]: the adjoint of ``corr_index_forward`` with respect to
    the volume (every element written, zeros included)."""
    _contiguous(volume=volume, coords=coords, corr_grad=corr_grad)
    dev = _device_of(volume=volume, coords=coords, corr_grad=corr_grad)
    n, h1, w1, h2, w2 = _lookup_shapes(volume, coords)
    r = int(radius)
    if corr_grad.dtype != volume.dtype or tuple(corr_grad.shape) != (n, 2 * r + 1, 2 * r + 1, h1, w1):
        raise RuntimeError("corr_grad must have the volume's dtype and dimensions (n, 2r+1, 2r+1, h1, w1)")
    volume_grad = torch.empty_like(volume)
    if volume_grad.numel() == 0:
        return [volume_grad]
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_corr_index_backward(coords.data_ptr(), corr_grad.data_ptr(),
                                                    _DTYPE_TAG[volume.dtype], n, h1, w1, h2, w2, r,
                                                    volume_grad.data_ptr(), _lib.stream_handle(dev)))
    return [volume_grad]


def _not_built(name):
    def op(*args, **kwargs):
        raise NotImplementedError(f"droid_backends.{name} is not built for MI355X yet (csrc/droid.hip has "
                                  f"frame_distance, depth_filter, iproj and corr_index_*)")
    op.__name__ = name
    return op


ba = _not_built("ba")
projmap = _not_built("projmap")
altcorr_forward = _not_built("altcorr_forward")
altcorr_backward = _not_built("altcorr_backward")
