"""``droid_backends`` on MI355X: the native module the reference imports in
``src/depth_video.py`` and ``src/modules/droid_net/corr.py``
(bindings: src/lib/droid.cpp:254-266), computed by libwgsr.so's gfx950
kernels (csrc/droid*.hip, include/wgsr.h ``wgsr_droid_*``).

Built: ``ba`` (csrc/droid_ba.hip), ``frame_distance``, ``depth_filter``,
``iproj``, ``corr_index_forward``, ``corr_index_backward``, and
``altcorr_forward`` / ``altcorr_backward`` (csrc/droid_altcorr.hip: the
lookups of the backend's ``FactorGraph.update_lowmem``) -- the reference's
argument order and return shapes (the lookups return lists).
Not built: ``projmap``, which the reference's Python never calls; it raises
``NotImplementedError`` naming the op.  Launches go on torch's current stream.
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


# ---------------------------------------------------------------------------
# bundle adjustment
# ---------------------------------------------------------------------------
BA_STATUS = {1: "an ii or jj entry lies outside [0, num)",      # WGSR_BA_BAD_INDEX
             2: "a jj entry is >= t1",                          # WGSR_BA_BAD_JJ
             4: "eta's rows do not match the frames {t0..t1-1} u set(ii)"}  # WGSR_BA_BAD_K


def _ba_prepare(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, t0, t1):
    """The shared checks of ``ba`` and ``_ba_system``: (device, num, ht, wd,
    n_edges, K, t0, t1, workspace, status)."""
    tensors = dict(poses=poses, disps=disps, intrinsics=intrinsics, disps_sens=disps_sens, targets=targets,
                   weights=weights, eta=eta, ii=ii, jj=jj)
    _contiguous(**tensors)
    dev = _device_of(**tensors)
    num, ht, wd = _frames(poses, disps, intrinsics)
    _index("ii", ii)
    _index("jj", jj)
    n = ii.numel()
    if jj.numel() != n:
        raise RuntimeError("ii and jj must have the same length")
    for name, t in (("disps_sens", disps_sens), ("targets", targets), ("weights", weights), ("eta", eta)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32")
    if disps_sens.dim() != 3 or disps_sens.size(0) < num or tuple(disps_sens.shape[1:]) != (ht, wd):
        raise RuntimeError("disps_sens must have dimensions (num, ht, wd)")
    if tuple(targets.shape) != (n, 2, ht, wd) or tuple(weights.shape) != (n, 2, ht, wd):
        raise RuntimeError("targets and weights must have dimensions (n_edges, 2, ht, wd)")
    if eta.dim() != 3 or tuple(eta.shape[1:]) != (ht, wd):
        raise RuntimeError("eta must have dimensions (K, ht, wd)")
    t0, t1, K = int(t0), int(t1), eta.size(0)
    L = _lib.load()
    nbytes = L.wgsr_droid_ba_workspace_bytes(num, ht, wd, n, t0, t1, K)
    if nbytes < 0:
        _lib.check(1)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    return dev, num, ht, wd, n, K, t0, t1, workspace, status


def _ba_raise(status):
    word = int(status.item())
    if word:
        what = "; ".join(msg for bit, msg in BA_STATUS.items() if word & bit)
        raise RuntimeError(f"droid_backends.ba: {what} (status {word}); poses and disps are unchanged")


def _ba(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, t0, t1, iterations, lm, ep,
        motion_only, depth_only, check=True):
    dev, num, ht, wd, n, K, t0, t1, workspace, status = _ba_prepare(poses, disps, intrinsics, disps_sens, targets,
                                                                     weights, eta, ii, jj, t0, t1)
    motion_only = bool(motion_only)
    dx = torch.zeros(t1 - t0, 6, dtype=torch.float32, device=dev)
    dz = torch.zeros((0,) if motion_only else (K, ht * wd), dtype=torch.float32, device=dev)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_ba(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), disps_sens.data_ptr(),
                                   targets.data_ptr(), weights.data_ptr(), eta.data_ptr(), ii.data_ptr(),
                                   jj.data_ptr(), num, ht, wd, n, K, t0, t1, int(iterations), float(lm), float(ep),
                                   int(motion_only), int(bool(depth_only)), workspace.data_ptr(), workspace.numel(),
                                   dx.data_ptr(), None if motion_only else dz.data_ptr(), status.data_ptr(),
                                   _lib.stream_handle(dev)))
    if check:
        _ba_raise(status)
    return [dx, dz]


def ba(*args, **kwargs):
    """[dx [P, 6], dz [K, ht * wd]]: ``iterations`` Gauss-Newton steps of the
    dense bundle adjustment; ``poses[t0:t1]`` and the disparities of the
    frames {t0..t1-1} u set(ii) are updated in place (``motion_only``: poses
    only, ``dz`` empty; ``depth_only``: disparities only).  The reference's
    call form: ``ba(poses, disps, intrinsics, disps_sens, targets, weights,
    eta, ii, jj, t0, t1, iterations, lm, ep, motion_only, depth_only)``.

    The kernels validate the indices on the device; by default the status
    word is read back after the call and a ``RuntimeError`` names what was
    wrong (poses and disps are then unchanged).  ``check=False`` skips that
    read: the call then makes no synchronisation and can be captured in a
    graph."""
    if len(args) != 16 or set(kwargs) - {"check"}:
        raise NotImplementedError("droid_backends.ba: only the reference's call form (poses, disps, ..., depth_only) "
                                  "is implemented")
    return _ba(*args, **kwargs)


def _ba_system(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, t0, t1, lm, ep,
               motion_only=False, check=True):
    """Diagnostic: one linearisation at the current state, nothing updated.
    (H [6P, 6P], g [6P]) in float64 = the damped reduced system, C and w
    [K, ht * wd] (None with ``motion_only``), and the solve's dx [P, 6]."""
    dev, num, ht, wd, n, K, t0, t1, workspace, status = _ba_prepare(poses, disps, intrinsics, disps_sens, targets,
                                                                     weights, eta, ii, jj, t0, t1)
    motion_only = bool(motion_only)
    P = t1 - t0
    H = torch.zeros(6 * P, 6 * P, dtype=torch.float64, device=dev)
    g = torch.zeros(6 * P, dtype=torch.float64, device=dev)
    dx = torch.zeros(P, 6, dtype=torch.float32, device=dev)
    C = w = None
    if not motion_only:
        C = torch.zeros(K, ht * wd, dtype=torch.float32, device=dev)
        w = torch.zeros(K, ht * wd, dtype=torch.float32, device=dev)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_ba_system(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(),
                                          disps_sens.data_ptr(), targets.data_ptr(), weights.data_ptr(),
                                          eta.data_ptr(), ii.data_ptr(), jj.data_ptr(), num, ht, wd, n, K, t0, t1,
                                          float(lm), float(ep), int(motion_only), workspace.data_ptr(),
                                          workspace.numel(), H.data_ptr(), g.data_ptr(),
                                          None if motion_only else C.data_ptr(),
                                          None if motion_only else w.data_ptr(), dx.data_ptr(), status.data_ptr(),
                                          _lib.stream_handle(dev)))
    if check:
        _ba_raise(status)
    return H, g, C, w, dx


# ---------------------------------------------------------------------------
# on-the-fly correlation
# ---------------------------------------------------------------------------
def _altcorr_shapes(fmap1, fmap2, coords, dtypes):
    if fmap1.dim() != 4 or fmap2.dim() != 4:
        raise RuntimeError("fmap1 and fmap2 must have dimensions (b, h, w, c), channels last")
    if fmap1.dtype not in dtypes or fmap2.dtype != fmap1.dtype:
        names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise RuntimeError(f"fmap1 and fmap2 must both be {names}, got {fmap1.dtype} and {fmap2.dtype}")
    if fmap2.size(3) != fmap1.size(3) or fmap1.size(3) <= 0 or fmap1.size(3) % 32 != 0:
        raise RuntimeError("fmap1 and fmap2 must have the same channel count, a positive multiple of 32")
    if coords.dim() != 5 or coords.dtype != torch.float32 or coords.size(4) != 2:
        raise RuntimeError("coords must be a float32 tensor of dimensions (b, n, h1, w1, 2)")
    return coords.size(0), coords.size(1), fmap1.size(1), fmap1.size(2), fmap2.size(1), fmap2.size(2), fmap1.size(3)


def _altcorr_launch(fmap1, fmap2, coords, ii, jj, radius, coord_scale, out, channel_offset, dev):
    """One forward launch into ``out`` [b, n, channels, h1, w1] (contiguous) at
    ``channel_offset``; entry e reads fmap1[ii[e]] and fmap2[jj[e]] (``None``:
    map e).  Shared by ``altcorr_forward`` and ``wgsr.frontend.AltCorrBlock``."""
    b, n, h1, w1 = coords.shape[:4]
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_altcorr_forward(
            fmap1.data_ptr(), fmap2.data_ptr(), coords.data_ptr(), None if ii is None else ii.data_ptr(),
            None if jj is None else jj.data_ptr(), _DTYPE_TAG[fmap1.dtype], _DTYPE_TAG[out.dtype], fmap1.size(0),
            fmap2.size(0), b, n, h1, w1, fmap2.size(1), fmap2.size(2), fmap1.size(3), int(radius),
            float(coord_scale), out.data_ptr(), out.stride(0), out.stride(1), int(channel_offset),
            _lib.stream_handle(dev)))


def _altcorr_forward(fmap1, fmap2, coords, radius):
    _contiguous(fmap1=fmap1, fmap2=fmap2, coords=coords)
    b, n, h1, w1, h2, w2, c = _altcorr_shapes(fmap1, fmap2, coords, (torch.float32, torch.float16))
    dev = _device_of(fmap1=fmap1, fmap2=fmap2, coords=coords)
    if fmap1.size(0) != b or fmap2.size(0) != b or tuple(coords.shape[2:4]) != (h1, w1):
        raise RuntimeError("fmap1 (b, h1, w1, c), fmap2 (b, h2, w2, c) and coords (b, n, h1, w1, 2) do not match")
    r = int(radius)
    corr = torch.empty(b, n, (2 * r + 1) ** 2, h1, w1, dtype=fmap1.dtype, device=dev)
    if corr.numel() == 0:
        return [corr]
    _altcorr_launch(fmap1, fmap2, coords, None, None, r, 1.0, corr, 0, dev)
    return [corr]


def _altcorr_backward(fmap1, fmap2, coords, corr_grad, radius):
    _contiguous(fmap1=fmap1, fmap2=fmap2, coords=coords, corr_grad=corr_grad)
    b, n, h1, w1, h2, w2, c = _altcorr_shapes(fmap1, fmap2, coords, (torch.float32,))
    dev = _device_of(fmap1=fmap1, fmap2=fmap2, coords=coords, corr_grad=corr_grad)
    if fmap1.size(0) != b or fmap2.size(0) != b or tuple(coords.shape[2:4]) != (h1, w1):
        raise RuntimeError("fmap1 (b, h1, w1, c), fmap2 (b, h2, w2, c) and coords (b, n, h1, w1, 2) do not match")
    r = int(radius)
    if corr_grad.dtype != torch.float32 or tuple(corr_grad.shape) != (b, n, (2 * r + 1) ** 2, h1, w1):
        raise RuntimeError("corr_grad must be a float32 tensor of dimensions (b, n, (2r+1)^2, h1, w1)")
    fmap1_grad = torch.empty_like(fmap1)
    fmap2_grad = torch.empty_like(fmap2)
    coords_grad = torch.empty_like(coords)
    if b == 0:
        return [fmap1_grad, fmap2_grad, coords_grad]
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_altcorr_backward(fmap1.data_ptr(), fmap2.data_ptr(), _lib.ptr(coords),
                                                 _lib.ptr(corr_grad), b, n, h1, w1, h2, w2, c, r,
                                                 fmap1_grad.data_ptr(), fmap2_grad.data_ptr(), _lib.ptr(coords_grad),
                                                 _lib.stream_handle(dev)))
    return [fmap1_grad, fmap2_grad, coords_grad]


def altcorr_forward(*args, **kwargs):
    """[corr [b, n, (2r+1)^2, h1, w1]]: the correlation lookup computed on the
    fly (CorrLayer.forward).  ``fmap1`` [b, h1, w1, c] and ``fmap2`` [b, h2,
    w2, c] channels last, float32 or float16 (corr has their type, accumulated
    in fp32); ``coords`` [b, n, h1, w1, 2] float32 (x, y).  corr[b, n, iy +
    (2r+1) ix] is the bilinear sample, at (x + ix - r, y + iy - r), of the
    pixel's dot products with ``fmap2``: ``corr_index_forward`` of the
    all-pairs volume, which is never stored.  c a positive multiple of 32."""
    if len(args) != 4 or kwargs:
        raise NotImplementedError("droid_backends.altcorr_forward: only the reference's call form "
                                  "(fmap1, fmap2, coords, radius) is implemented")
    return _altcorr_forward(*args)


def altcorr_backward(*args, **kwargs):
    """[fmap1_grad, fmap2_grad, coords_grad] of ``altcorr_forward`` (float32
    only): the adjoint of the forward with respect to the two maps;
    ``coords_grad`` is all zeros, as in the reference.  ``fmap2_grad`` is
    accumulated with atomic adds and is not bit-reproducible."""
    if len(args) != 5 or kwargs:
        raise NotImplementedError("droid_backends.altcorr_backward: only the reference's call form "
                                  "(fmap1, fmap2, coords, corr_grad, radius) is implemented")
    return _altcorr_backward(*args)


def projmap(*args, **kwargs):
    raise NotImplementedError("droid_backends.projmap is not built for MI355X (the reference's Python never calls "
                              "it); every other name of the module is: csrc/droid.hip, csrc/droid_altcorr.hip, "
                              "csrc/droid_ba.hip")
