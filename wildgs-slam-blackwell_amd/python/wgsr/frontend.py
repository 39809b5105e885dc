"""What the mapper reads from the tracker's ``DepthVideo``, over the
``droid_backends`` kernels (csrc/droid.hip) and without ``lietorch``:

* ``distance``          DepthVideo.distance (depth_video.py:205-235)
* ``valid_depth_mask``  DepthVideo.update_valid_depth_mask (depth_video.py:407-442)
* ``depth_and_pose``    the non-metric branch of DepthVideo.get_depth_and_pose
                        with get_w2c_and_depth's validity flag (mapper.py:574-599)
* ``ba``                DepthVideo.ba (depth_video.py:351-373): the dense bundle
                        adjustment (csrc/droid_ba.hip)
* ``AltCorrBlock``      the correlation lookups of FactorGraph.update_lowmem
                        (corr.py AltCorrBlock), one fused launch per pyramid
                        level (csrc/droid_altcorr.hip)
* ``CorrBlock``         the all-pairs correlation pyramid of the frontend's local
                        graph and the motion filter (corr.py CorrBlock): the
                        volume and its pooled levels in one launch into the
                        slots of a store, every level looked up in one launch
                        (csrc/droid_corrvol.hip)
* ``reproject``         DepthVideo.reproject / projective_ops.projective_transform
                        (projective_ops.py:110-139), one fused launch
                        (csrc/lie.hip) instead of the composition of group ops
* ``upsample``          DepthVideo.upsample (depth_video.py:179-183): the convex
                        upsampling of the disparities in place on the video
                        buffers, one launch (csrc/droid_upsample.hip), with
                        ``cvx_upsample`` / ``upsample_disp`` (droid_net.py:23-45)
                        and ``upsample_from_features``, which computes the mask
                        head (GraphAgg.upmask) inside the same launch
* ``update_heads``      UpdateModule's delta and weight heads (droid_net.py:
                        102-115, 141-145) and ``graph_agg``, GraphAgg.forward up
                        to eta and the features of upmask (droid_net.py:65-77):
                        3 x 3 convolutions on one fp16 MFMA implicit-GEMM kernel
                        (csrc/droid_conv3x3.hip); ``pack_conv3x3`` packs a
                        convolution's parameters for it
* ``conv_gru``          UpdateModule's ConvGRU (gru.py:34-48, droid_net.py:138):
                        the glo term, then the z / r and the q convolutions over
                        [net, inp, corr, flow] on the wide-K form of that kernel,
                        the concatenations never written (csrc/droid_gru.hip);
                        ``pack_conv3x3_wide`` packs a convolution of any C_in
                        that is a multiple of 32
* ``corr_encoder``      UpdateModule's corr and flow encoders (droid_net.py:88-100,
  ``flow_encoder``      136-137): one launch each, the first layer's float16
                        result kept in LDS for the 3 x 3 layer
                        (csrc/droid_encoders.hip)
* ``update_operator``   the whole UpdateModule.forward (droid_net.py:120-153): the
                        composition of the calls above
* ``feature_encoder``   DroidNet.fnet / .cnet (the BasicEncoder of extractor.py:
  ``context_encoder``   75-141; motion_filter.py:39-48, 61-70): 14 convolution
                        launches that write each raw map once and apply the
                        norm, the ReLU and the residual sum as the next launch
                        stages its tile (csrc/droid_basic_encoder.hip)
* ``filter_mono_depth`` DepthVideo.filter_high_err_mono_depth (depth_video.py:
                        281-349): the DINO-consistency filter of the metric
                        depth prior from fp32 MFMA Gram matrices of the cell
                        maps, no full-resolution feature map
                        (csrc/droid_mono_filter.hip)

poses [num, 7] = (tx, ty, tz, qx, qy, qz, qw), world to camera; disps
[num, ht, wd]; intrinsics [4] = (fx, fy, cx, cy); device fp32 tensors.
"""
from __future__ import annotations

import heapq
import weakref

import torch
import torch.nn.functional as F

import droid_backends
from wgsr import _lib

MIN_VALID_DEPTHS = 100  # mapper.py:593
REPROJECT_JACOBIAN, REPROJECT_DEPTH = 1, 2  # WGSR_REPROJECT_* (include/wgsr.h)


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


@torch.no_grad()
def reproject(poses, disps, intrinsics, ii, jj, jacobian=False, return_depth=False, check=True):
    """projective_ops.projective_transform on the video buffers: ``poses``
    [num, 7], ``disps`` [num, ht, wd], ``intrinsics`` [num, 4] (or one [4]),
    ``ii`` / ``jj`` [E] int64, all on the device.  Returns the reference's
    shapes: ``coords`` [1, E, ht, wd, 2] (3 with ``return_depth``: disparity
    over depth in the third slot), ``valid`` [1, E, ht, wd, 1] (0 / 1 floats,
    depth > 0.2) and, with ``jacobian``, ``(Ji, Jj, Jz)`` [1, E, ht, wd, 2, 6 |
    6 | 1].  ``check`` reads ``ii.max()`` / ``jj.max()`` on the host and raises
    for an index outside [0, num); with ``check=False`` there is no host read
    (the call can be captured in a graph) and such an edge's outputs are NaN."""
    droid_backends._contiguous(poses=poses, disps=disps, intrinsics=intrinsics, ii=ii, jj=jj)
    dev = droid_backends._device_of(poses=poses, disps=disps, intrinsics=intrinsics, ii=ii, jj=jj)
    if poses.dim() != 2 or poses.size(1) != 7:
        raise RuntimeError("poses must have dimensions (num, 7)")
    if disps.dim() != 3:
        raise RuntimeError("disps must have dimensions (num, ht, wd)")
    num, ht, wd = min(poses.size(0), disps.size(0)), disps.size(1), disps.size(2)
    per_frame = intrinsics.dim() == 2
    if per_frame:
        if intrinsics.size(1) != 4:
            raise RuntimeError("intrinsics must have dimensions (num, 4) or (4,)")
        num = min(num, intrinsics.size(0))
    elif tuple(intrinsics.shape) != (4,):
        raise RuntimeError("intrinsics must have dimensions (num, 4) or (4,)")
    for name, t in (("poses", poses), ("disps", disps), ("intrinsics", intrinsics)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32")
    droid_backends._index("ii", ii)
    droid_backends._index("jj", jj)
    if ii.numel() != jj.numel():
        raise RuntimeError("ii and jj must have the same length")
    E = ii.numel()
    coords = torch.empty(1, E, ht, wd, 3 if return_depth else 2, dtype=torch.float32, device=dev)
    valid = torch.empty(1, E, ht, wd, 1, dtype=torch.float32, device=dev)
    Ji = Jj = Jz = None
    if jacobian:
        Ji = torch.empty(1, E, ht, wd, 2, 6, dtype=torch.float32, device=dev)
        Jj = torch.empty_like(Ji)
        Jz = torch.empty(1, E, ht, wd, 2, 1, dtype=torch.float32, device=dev)
    if E and coords.numel():
        if check:
            lo = int(min(ii.min().item(), jj.min().item()))
            hi = int(max(ii.max().item(), jj.max().item()))
            if lo < 0 or hi >= num:
                raise RuntimeError(f"ii / jj must index frames [0, {num}): got values in [{lo}, {hi}]")
        flags = (REPROJECT_JACOBIAN if jacobian else 0) | (REPROJECT_DEPTH if return_depth else 0)
        L = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(L.wgsr_droid_reproject(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(),
                                              int(per_frame), num, ht, wd, ii.data_ptr(), jj.data_ptr(), E, flags,
                                              coords.data_ptr(), valid.data_ptr(), _lib.ptr(Ji), _lib.ptr(Jj),
                                              _lib.ptr(Jz), _lib.stream_handle(dev)))
    if jacobian:
        return coords, valid, (Ji, Jj, Jz)
    return coords, valid


class AltCorrBlock:
    """The on-the-fly correlation pyramid of the global bundle adjustment's
    update loop.  ``fmaps`` [B, N, C, H, W] (any float type; the video buffer's
    is float16) become ``pyramid``: ``num_levels`` channels-last maps [B, N,
    H // 2^i, W // 2^i, C] of ``fmaps`` / 4, each level the 2 x 2 average of
    the one before, in ``fmaps``' own type.

    ``block(coords, ii, jj)`` with ``coords`` [B, E, H, W, 2] (x, y) and frame
    indices ``ii``, ``jj`` [E] returns float32 [B, E, num_levels (2r+1)^2, H,
    W]: for level i the lookup of frame ii's level-0 features in frame jj's
    level-i map around ``coords`` / 2^i.  Each level is one launch that reads
    the pyramid in place through the index arrays (batch b reads map b N +
    ii), converts on load, scales the coordinates itself and writes its
    channel slice of the result: no per-edge copies of the maps, no
    concatenation.  ``coords`` [B, E, H, W, S, 2] gives [B, E, num_levels
    (2r+1)^2, H, W, S].

    Inference only: the result carries no autograd graph.  Training goes
    through ``droid_backends.altcorr_forward`` / ``altcorr_backward``."""

    def __init__(self, fmaps, num_levels=4, radius=3):
        self.num_levels = num_levels
        self.radius = radius
        B, N, C, H, W = fmaps.shape
        level = fmaps.reshape(B * N, C, H, W) / 4.0
        self.pyramid = []
        for i in range(num_levels):
            self.pyramid.append(level.permute(0, 2, 3, 1).contiguous().view(B, N, H // 2 ** i, W // 2 ** i, C))
            if i + 1 < num_levels:
                level = F.avg_pool2d(level, kernel_size=2, stride=2)

    @torch.no_grad()
    def __call__(self, coords, ii, jj):
        samples = coords.dim() == 6
        if coords.dim() not in (5, 6) or coords.size(-1) != 2 or coords.dtype != torch.float32:
            raise RuntimeError("coords must be a float32 tensor of dimensions (B, E, H, W, 2) or (B, E, H, W, S, 2)")
        B, N, H, W, C = self.pyramid[0].shape
        if self.pyramid[0].dtype not in (torch.float32, torch.float16) or C % 32 != 0:
            raise RuntimeError("the feature maps must be float32 or float16 with a multiple of 32 channels")
        dev =droid_backends._device_of(coords=coords, fmaps=self.pyramid[0])
        E = coords.size(1)
        if coords.size(0) != B or tuple(coords.shape[2:4]) != (H, W):
            raise RuntimeError("coords must have the feature maps' batch size, height and width")
        S = coords.size(4) if samples else 1
        # the kernel's coords are [entries, samples, H, W, 2]
        if samples:
            coords = coords.permute(0, 1, 4, 2, 3, 5)
        coords = coords.reshape(B * E, S, H, W, 2).contiguous()
        index = []
        for name, t in (("ii", ii), ("jj", jj)):
            t = torch.as_tensor(t).to(dev, torch.int64).reshape(-1)
            if t.numel() != E:
                raise RuntimeError(f"{name} must have one frame index per edge")
            if B > 1:
                t = (torch.arange(B, device=dev)[:, None] * N + t[None]).reshape(-1)
            index.append(t.contiguous())
        rd2 = (2 * self.radius + 1) ** 2
        out = torch.empty(B * E, S, self.num_levels * rd2, H, W, dtype=torch.float32, device=dev)
        if out.numel():
            fmap1 = self.pyramid[0].view(B * N, H, W, C)
            for i, level in enumerate(self.pyramid):
                droid_backends._altcorr_launch(fmap1, level.view((B * N,) + level.shape[2:]), coords, index[0],
                                               index[1], self.radius, 2.0 ** -i, out, i * rd2, dev)
        if samples:
            return out.view(B, E, S, -1, H, W).permute(0, 1, 3, 4, 5, 2).contiguous()
        return out.view(B, E, -1, H, W)


# ---------------------------------------------------------------------------
# CorrBlock: the all-pairs correlation pyramid, held in slots
# ---------------------------------------------------------------------------
CORR_MAX_LEVELS = 4  # kCvMaxLevels (csrc/droid_corrvol.hip)


def corr_slot_layout(h, w, num_levels):
    """(offsets, elems): the first fp16 element of each level in a slot and
    the elements per slot; every level starts on a 16-byte boundary
    (``wgsr_droid_corr_slot_bytes``)."""
    offsets, at = [], 0
    for i in range(num_levels):
        offsets.append(at)
        at += h * w * (h >> i) * (w >> i)
        at = (at + 7) & ~7
    return offsets, at


class SlotTable:
    """The bookkeeping of a slot store, on the host and without a device: the
    free list and the table edge -> slot, in edge order.  Free slots are taken
    lowest first; a full store grows by doubling."""

    def __init__(self, capacity):
        if capacity < 1:
            raise ValueError("a slot store needs a capacity of at least 1")
        self.capacity = int(capacity)
        self.slots = []                       # slot of edge k
        self._free = list(range(self.capacity))  # a heap

    def __len__(self):
        return len(self.slots)

    @property
    def free(self):
        return len(self._free)

    def grow(self, need):
        """Double the capacity until ``need`` slots are free."""
        while len(self._free) < need:
            for s in range(self.capacity, 2 * self.capacity):
                heapq.heappush(self._free, s)
            self.capacity *= 2
        return self.capacity

    def take(self, n):
        """n free slots (growing first if need be), appended to the table as
        the slots of n new edges."""
        self.grow(n)
        new = [heapq.heappop(self._free) for _ in range(n)]
        self.slots.extend(new)
        return new

    def release(self, slots):
        for s in slots:
            heapq.heappush(self._free, s)

    def select(self, index):
        """``table = table[index]`` for whatever indexes dimension 0 of a
        tensor (a boolean mask, an integer tensor, a slice); the slots no edge
        holds any more go back to the free list."""
        if isinstance(index, torch.Tensor):
            index = index.cpu()  # (a device mask: the one host read)
        kept = torch.tensor(self.slots, dtype=torch.int64)[index].reshape(-1).tolist()
        self.release(sorted(set(self.slots) - set(kept)))
        self.slots = kept
        return list(kept)


def _corr_geometry(store, slots, h, w, num_levels):
    L = _lib.load()
    slot_bytes = L.wgsr_droid_corr_slot_bytes(h, w, num_levels)
    if slot_bytes < 0:
        _lib.check(1)
    if store.dtype != torch.float16 or store.dim() != 1 or not store.is_contiguous():
        raise RuntimeError("the store must be a contiguous 1-D float16 tensor")
    if slots.dtype != torch.int32 or slots.dim() != 1 or not slots.is_contiguous():
        raise RuntimeError("slots must be a contiguous 1-D int32 tensor")
    return L, store.numel() // (slot_bytes // 2)


@torch.no_grad()
def corr_build(fmap1, fmap2, store, slots, num_levels=4):
    """Build the pyramids of n edges, ``fmap1`` / ``fmap2`` [n, C, H, W]
    float16, into slots ``slots`` [n] (device int32) of ``store`` (1-D
    float16, a whole number of slots): one launch, nothing read on the host."""
    droid_backends._contiguous(fmap1=fmap1, fmap2=fmap2)
    dev = droid_backends._device_of(fmap1=fmap1, fmap2=fmap2, store=store, slots=slots)
    if fmap1.dim() != 4 or fmap1.shape != fmap2.shape:
        raise RuntimeError("fmap1 and fmap2 must have the same dimensions (n, C, H, W)")
    if fmap1.dtype != torch.float16 or fmap2.dtype != torch.float16:
        raise NotImplementedError(f"corr_build: only float16 maps are built, got {fmap1.dtype} / {fmap2.dtype}")
    n, c, h, w = fmap1.shape
    L, capacity = _corr_geometry(store, slots, h, w, num_levels)
    if slots.numel() != n:
        raise RuntimeError("slots must name one slot per edge")
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_corr_build(fmap1.data_ptr(), fmap2.data_ptr(), droid_backends._DTYPE_TAG[fmap1.dtype],
                                           n, c, h, w, num_levels, store.data_ptr(), capacity, slots.data_ptr(),
                                           _lib.stream_handle(dev)))


@torch.no_grad()
def corr_lookup(store, slots, coords, num_levels=4, radius=3):
    """corr [n, num_levels (2r+1)^2, H, W] float16 of ``coords`` [n, H, W, 2]
    float32 (x, y): every level of the edges in ``slots`` in one launch."""
    droid_backends._contiguous(coords=coords)
    dev = droid_backends._device_of(store=store, slots=slots, coords=coords)
    if coords.dim() != 4 or coords.size(3) != 2 or coords.dtype != torch.float32:
        raise RuntimeError("coords must be a float32 tensor of dimensions (n, H, W, 2)")
    n, h, w, _ = coords.shape
    L, capacity = _corr_geometry(store, slots, h, w, num_levels)
    if slots.numel() != n:
        raise RuntimeError("slots must name one slot per edge")
    r = int(radius)
    out = torch.empty(n, num_levels * (2 * r + 1) ** 2, h, w, dtype=torch.float16, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_corr_lookup(store.data_ptr(), capacity, slots.data_ptr(), coords.data_ptr(),
                                            droid_backends._DTYPE_TAG[store.dtype], n, h, w, num_levels, r,
                                            out.data_ptr(), _lib.stream_handle(dev)))
    return out


class CorrBlock:
    """The reference's ``CorrBlock`` (corr.py:39-90) for inference, as the
    frontend's factor graph and the motion filter use it under autocast.
    ``fmap1``, ``fmap2`` [B, N, C, H, W] float16 give B N edges; an edge's
    pyramid -- level 0 [H, W, H, W] = fmap1 / 4 . fmap2 / 4 over the channels,
    level i + 1 the 2 x 2 average of level i as stored -- lives in one slot of
    a store, one device allocation of ``capacity`` slots (default: the edges
    given; size it once with e.g. ``max_factors`` plus a batch of new edges).

    ``block(coords)``, ``coords`` [B, N, H, W, 2]: float16 [B, N, num_levels
    (2r+1)^2, H, W] from one launch.  ``block.append(fmap1, fmap2)`` builds new
    edges straight into free slots (the store doubles when full);
    ``block.cat(other)`` copies ``other``'s edges into free slots and returns
    self; ``block[index]`` keeps the indexed edges by editing the slot table
    alone -- no volume moves -- and returns self.  ``corr_pyramid`` gathers the
    reference's list of [B N, H, W, H >> i, W >> i] tensors in edge order.

    Inference only: float32 maps, or an input that requires grad under grad
    mode, raise ``NotImplementedError``; training keeps the reference's torch
    composition over ``droid_backends.corr_index_forward`` / ``_backward``."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=3, capacity=None):
        self.num_levels = int(num_levels)
        self.radius = int(radius)
        if not 1 <= self.num_levels <= CORR_MAX_LEVELS:
            raise RuntimeError(f"num_levels must lie in [1, {CORR_MAX_LEVELS}]")
        edges, self.channels, self.ht, self.wd, dev = self._check_maps(fmap1, fmap2, first=True)
        self._offsets, self.slot_elems = corr_slot_layout(self.ht, self.wd, self.num_levels)
        self._table = SlotTable(max(edges, 1) if capacity is None else capacity)
        self._store = torch.empty(self._table.capacity * self.slot_elems, dtype=torch.float16, device=dev)
        self._slots_dev = None  # the device copy of the table, made when next needed
        self.append(fmap1, fmap2)

    def _check_maps(self, fmap1, fmap2, first=False):
        if fmap1.dim() != 5 or fmap1.shape != fmap2.shape:
            raise RuntimeError("fmap1 and fmap2 must have the same dimensions (B, N, C, H, W)")
        B, N, C, H, W = fmap1.shape
        if not first and (C, H, W) != (self.channels, self.ht, self.wd):
            raise RuntimeError(f"the maps must be (C, H, W) = ({self.channels}, {self.ht}, {self.wd}) like the "
                               f"block's, got ({C}, {H}, {W})")
        small = 1 << (self.num_levels - 1)
        if H < small or W < small:
            raise RuntimeError(f"H and W must each be at least {small} for {self.num_levels} levels, got {H} x {W}")
        if C % 32 != 0 or C == 0:
            raise RuntimeError(f"the channel count {C} must be a positive multiple of 32")
        for t in (fmap1, fmap2):
            if t.dtype != torch.float16:
                raise NotImplementedError(f"CorrBlock: only float16 maps are built (the tracker's autocast), got "
                                          f"{t.dtype}")
        if torch.is_grad_enabled() and (fmap1.requires_grad or fmap2.requires_grad):
            raise NotImplementedError("CorrBlock is inference only: an input requires grad (training keeps the torch "
                                      "composition)")
        dev = droid_backends._device_of(fmap1=fmap1, fmap2=fmap2)
        return B * N, C, H, W, dev

    # -- the store -----------------------------------------------------------
    def __len__(self):
        return len(self._table)

    @property
    def capacity(self):
        return self._table.capacity

    def _take(self, n):
        """Slots for n new edges; the store grows first if it is full (the
        held slots keep their numbers)."""
        new = self._table.take(n)
        if self._table.capacity * self.slot_elems != self._store.numel():
            store = torch.empty(self._table.capacity * self.slot_elems, dtype=torch.float16,
                                device=self._store.device)
            store[:self._store.numel()].copy_(self._store)
            self._store = store
        self._slots_dev = None
        return new

    def _slots(self):
        if self._slots_dev is None:
            self._slots_dev = torch.tensor(self._table.slots, dtype=torch.int32, device=self._store.device)
        return self._slots_dev

    @torch.no_grad()
    def append(self, fmap1, fmap2):
        """Build the edges of ``fmap1``, ``fmap2`` [B, N, C, H, W] into free
        slots, after the edges already held.  Returns self."""
        edges, C, H, W, dev = self._check_maps(fmap1, fmap2)
        if dev != self._store.device:
            raise RuntimeError(f"fmap1: expected a tensor on {self._store.device}, got {dev}")
        if edges:
            f1 = fmap1.detach().reshape(edges, C, H, W).contiguous()
            f2 = fmap2.detach().reshape(edges, C, H, W).contiguous()
            slots = torch.tensor(self._take(edges), dtype=torch.int32, device=dev)
            corr_build(f1, f2, self._store, slots, self.num_levels)
        return self

    @torch.no_grad()
    def cat(self, other):
        if (other.num_levels, other.ht, other.wd) != (self.num_levels, self.ht, self.wd):
            raise RuntimeError("cat: the other block has another shape or number of levels")
        if other._store.device != self._store.device:
            raise RuntimeError("cat: the other block lives on another device")
        theirs = list(other._table.slots)
        if theirs:
            mine = self._take(len(theirs))
            dst = self._store.view(-1, self.slot_elems)
            src = other._store.view(-1, self.slot_elems)
            for d, s in zip(mine, theirs):
                dst[d].copy_(src[s])
        return self

    def __getitem__(self, index):
        self._table.select(index)
        self._slots_dev = None
        return self

    @property
    def corr_pyramid(self):
        slots = self._slots().long()
        rows = self._store.view(-1, self.slot_elems)
        H, W = self.ht, self.wd
        return [rows[:, off:off + H * W * (H >> i) * (W >> i)].index_select(0, slots).view(-1, H, W, H >> i, W >> i)
                for i, off in enumerate(self._offsets)]

    @torch.no_grad()
    def __call__(self, coords):
        if coords.dim() != 5 or coords.size(-1) != 2 or coords.dtype != torch.float32:
            raise RuntimeError("coords must be a float32 tensor of dimensions (B, N, H, W, 2)")
        B, N, H, W, _ = coords.shape
        if (H, W) != (self.ht, self.wd) or B * N != len(self._table):
            raise RuntimeError(f"coords must be (B, N, {self.ht}, {self.wd}, 2) with B N = {len(self._table)} edges, "
                               f"got {tuple(coords.shape)}")
        droid_backends._device_of(coords=coords)
        out = corr_lookup(self._store, self._slots(), coords.reshape(B * N, H, W, 2).contiguous(), self.num_levels,
                          self.radius)
        return out.view(B, N, -1, H, W)


# ---------------------------------------------------------------------------
# Convex upsampling (csrc/droid_upsample.hip)
# ---------------------------------------------------------------------------
UPSAMPLE_MASK_CHANNELS = 576  # 9 neighbours x 8 x 8 sub-positions
UPSAMPLE_MAX_DIM = 4          # kUpMaxDim
UPSAMPLE_STATUS = {1: "an index is outside the source frames (WGSR_UPSAMPLE_BAD_SRC)",
                   2: "an index is outside the output frames (WGSR_UPSAMPLE_BAD_OUT)"}


def _inference_only(who, **tensors):
    if torch.is_grad_enabled():
        for name, t in tensors.items():
            if t is not None and t.requires_grad:
                raise NotImplementedError(f"{who} is inference only: {name} requires grad (training keeps the torch "
                                          "composition)")


def _upsample_mask(mask, n, ht, wd):
    if mask.dtype not in droid_backends._DTYPE_TAG:
        raise NotImplementedError(f"mask must be float16 or float32, got {mask.dtype}")
    if mask.numel() != n * UPSAMPLE_MASK_CHANNELS * ht * wd:
        raise ValueError(f"mask must hold {UPSAMPLE_MASK_CHANNELS} channels for each of the {n} maps of {ht} x {wd}: "
                         f"got {tuple(mask.shape)}")
    droid_backends._contiguous(mask=mask)
    return mask


def _upsample_index(ix, dev):
    ix = torch.as_tensor(ix)
    if ix.device.type == "cuda" and ix.device != dev:
        raise RuntimeError(f"ix: expected a tensor on {dev}, got {ix.device}")
    return ix.to(dev, torch.int64).reshape(-1).contiguous()


def _upsample_buffers(disps, disps_up):
    droid_backends._contiguous(disps=disps, disps_up=disps_up)
    dev = droid_backends._device_of(disps=disps, disps_up=disps_up)
    if disps.dim() != 3 or disps_up.dim() != 3 or disps.dtype != torch.float32 or disps_up.dtype != torch.float32:
        raise RuntimeError("disps and disps_up must be float32 tensors of dimensions (num, ht, wd) and (num, 8 ht, 8 wd)")
    ht, wd = disps.size(1), disps.size(2)
    if tuple(disps_up.shape[1:]) != (8 * ht, 8 * wd):
        raise ValueError(f"disps_up must be (num, {8 * ht}, {8 * wd}) for disps of {ht} x {wd}: got "
                         f"{tuple(disps_up.shape)}")
    return dev, ht, wd


def _raise_status(who, status, table):
    """Reads the status word back (one synchronisation); non-zero: ``RuntimeError`` with ``table``'s messages."""
    word = int(status.item())
    if word:
        what = "; ".join(msg for bit, msg in table.items() if word & bit)
        raise RuntimeError(f"{who}: {what} (status {word}); nothing was written")


def _cvx_launch(who, data, src_index, mask, out, out_index, n, dim, check, dev):
    status = torch.empty(1, dtype=torch.int32, device=dev)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_cvx_upsample(data.data_ptr(), _lib.ptr(src_index), mask.data_ptr(),
                                             droid_backends._DTYPE_TAG[mask.dtype], out.data_ptr(),
                                             _lib.ptr(out_index), n, data.size(0), out.size(0), data.size(1),
                                             data.size(2), dim, status.data_ptr(), _lib.stream_handle(dev)))
    if check:
        _raise_status(who, status, UPSAMPLE_STATUS)


def cvx_upsample(data, mask):
    """The reference's ``cvx_upsample`` (droid_net.py:23-37): ``data`` [n, ht,
    wd, dim] float32 (dim <= 4), ``mask`` n x 576 x ht x wd values (float16 or
    float32, any shape that views to it) -> [n, 8 ht, 8 wd, dim] float32: each
    fine pixel the softmax-weighted sum of the 3 x 3 coarse neighbourhood
    (zero-padded), the softmax in fp32, one launch."""
    _inference_only("cvx_upsample", data=data, mask=mask)
    dev = droid_backends._device_of(data=data, mask=mask)
    if data.dim() != 4 or data.dtype != torch.float32:
        raise RuntimeError("data must be a float32 tensor of dimensions (n, ht, wd, dim)")
    n, ht, wd, dim = data.shape
    if not 1 <= dim <= UPSAMPLE_MAX_DIM:
        raise NotImplementedError(f"data: dim = {dim} outside [1, {UPSAMPLE_MAX_DIM}] is not built")
    mask = _upsample_mask(mask.detach(), n, ht, wd)
    data = data.detach().contiguous()
    out = torch.empty(n, 8 * ht, 8 * wd, dim, dtype=torch.float32, device=dev)
    if out.numel():
        _cvx_launch("cvx_upsample", data, None, mask, out, None, n, dim, False, dev)
    return out


def upsample_disp(disp, mask):
    """The reference's ``upsample_disp`` (droid_net.py:40-45): ``disp`` [batch,
    num, ht, wd] -> [batch, num, 8 ht, 8 wd]."""
    if disp.dim() != 4:
        raise RuntimeError("disp must have dimensions (batch, num, ht, wd)")
    batch, num, ht, wd = disp.shape
    return cvx_upsample(disp.reshape(batch * num, ht, wd, 1), mask).view(batch, num, 8 * ht, 8 * wd)


def upsample(disps, disps_up, ix, mask, check=True):
    """DepthVideo.upsample on the video buffers: ``disps_up[ix] =
    cvx_upsample(disps[ix][..., None], mask)`` in one launch that reads the
    frames ``ix`` of ``disps`` [num, ht, wd] and writes the frames ``ix`` of
    ``disps_up`` [num, 8 ht, 8 wd] in place; no gathered copy, no scatter, the
    other frames untouched.  ``ix`` [n] int64 with distinct entries in any order
    (n = 1 included); ``mask`` the n x 576 x ht x wd outputs of the mask head,
    float16 or float32.  The kernel validates ``ix`` on the device; ``check``
    reads the status word back and raises ``RuntimeError`` for an index outside
    the buffers (``disps_up`` is then unchanged).  ``check=False`` skips that
    read: no synchronisation, and the call can be captured in a graph (``ix``
    then has to be a device tensor already)."""
    _inference_only("upsample", disps=disps, mask=mask)
    dev, ht, wd = _upsample_buffers(disps, disps_up)
    droid_backends._device_of(mask=mask)
    ix = _upsample_index(ix, dev)
    n = ix.numel()
    mask = _upsample_mask(mask.detach(), n, ht, wd)
    if n and disps_up[0].numel():
        _cvx_launch("upsample", disps.detach().unsqueeze(-1), ix, mask, disps_up.detach().unsqueeze(-1), ix, n, 1,
                    check, dev)


_HEAD_CACHE = {}    # (data_ptr, version, dtype, shape) of a parameter -> its kernel-ready copy
_HEAD_CACHE_MAX = 8


def _head_param(src, dtype, shape):
    """``src`` as a contiguous ``dtype`` tensor of ``shape``; a converted copy
    is kept until the parameter is written again (its version changes).  An
    entry also holds a weak reference to the tensor it was made from and
    serves that tensor only: the allocator hands a freed tensor's address, with
    version 0 again, to the next tensor of its size."""
    t = src.detach()
    if t.dtype == dtype and t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t.view(shape)
    key = (t.data_ptr(), t._version, t.dtype, tuple(t.shape), t.device)
    hit = _HEAD_CACHE.get(key)
    if hit is not None and hit[0]() is src:
        return hit[1]
    _HEAD_CACHE.pop(key, None)
    if len(_HEAD_CACHE) >= _HEAD_CACHE_MAX:
        _HEAD_CACHE.pop(next(iter(_HEAD_CACHE)))
    copy = t.reshape(shape).to(dtype).contiguous()
    _HEAD_CACHE[key] = (weakref.ref(src), copy)
    return copy


def upsample_from_features(disps, disps_up, ix, feat, weight, bias, check=True):
    """``upsample`` with the mask head inside the launch: ``feat`` [n, C, ht,
    wd] float16 (a leading batch dimension of 1 is accepted; C a multiple of
    32) is what ``GraphAgg`` feeds to ``self.upmask``, ``weight`` that
    ``Conv2d``'s [576, C, 1, 1] (or [576, C]) and ``bias`` its [576].  A logit
    is the fp32 MFMA sum over C plus the bias, rounded once to float16 -- the
    value the convolution hands on under autocast -- and never reaches memory.
    float32 parameters are converted once and the copy kept (keyed on the
    parameter's address and version)."""
    _inference_only("upsample_from_features", disps=disps, feat=feat, weight=weight, bias=bias)
    dev, ht, wd = _upsample_buffers(disps, disps_up)
    droid_backends._device_of(feat=feat, weight=weight, bias=bias)
    ix = _upsample_index(ix, dev)
    n = ix.numel()
    if feat.dtype != torch.float16:
        raise NotImplementedError(f"feat: only float16 features are built (the tracker's autocast), got {feat.dtype}")
    if feat.dim() == 5 and feat.size(0) == 1:
        feat = feat[0]
    if feat.dim() != 4 or feat.size(0) != n or tuple(feat.shape[2:]) != (ht, wd):
        raise ValueError(f"feat must be (n, C, ht, wd) = ({n}, C, {ht}, {wd}): got {tuple(feat.shape)}")
    C = feat.size(1)
    if C == 0 or C % 32 != 0:
        raise ValueError(f"feat: the channel count C = {C} must be a positive multiple of 32")
    if weight.dim() not in (2, 4) or weight.size(0) != UPSAMPLE_MASK_CHANNELS or weight.numel() != \
            UPSAMPLE_MASK_CHANNELS * C:
        raise ValueError(f"weight must be ({UPSAMPLE_MASK_CHANNELS}, {C}) or ({UPSAMPLE_MASK_CHANNELS}, {C}, 1, 1): "
                         f"got {tuple(weight.shape)}")
    if bias.numel() != UPSAMPLE_MASK_CHANNELS:
        raise ValueError(f"bias must hold {UPSAMPLE_MASK_CHANNELS} values: got {tuple(bias.shape)}")
    droid_backends._contiguous(feat=feat)
    w16 = _head_param(weight, torch.float16, (UPSAMPLE_MASK_CHANNELS, C))
    b32 = _head_param(bias, torch.float32, (UPSAMPLE_MASK_CHANNELS,))
    if not n or not disps_up[0].numel():
        return
    status = torch.empty(1, dtype=torch.int32, device=dev)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_upmask_upsample(feat.data_ptr(), w16.data_ptr(), b32.data_ptr(), C, disps.data_ptr(),
                                                ix.data_ptr(), disps_up.data_ptr(), ix.data_ptr(), n, disps.size(0),
                                                disps_up.size(0), ht, wd, status.data_ptr(),
                                                _lib.stream_handle(dev)))
    if check:
        _raise_status("upsample_from_features", status, UPSAMPLE_STATUS)


# ---------------------------------------------------------------------------
# The update operator's output heads and GraphAgg (csrc/droid_conv3x3.hip)
# ---------------------------------------------------------------------------
CONV3X3_CIN = 128            # kCvCin
GRAPH_AGG_STATUS = {1: "an entry of ix is outside [0, num_groups) (WGSR_GRAPH_AGG_BAD_IX)"}
_PACK_CACHE = {}    # the key of _cached -> (weak references to the parameters, what was made of them)
_PACK_CACHE_MAX = 16


def _cached(srcs, tag, make):
    """``make()`` of the parameters ``srcs``, kept under them and ``tag`` until one
    of them is written again, as ``_head_param`` keeps its copies."""
    key = tuple((t.data_ptr(), t._version, t.dtype, tuple(t.shape), t.device) for t in srcs) + tag
    hit = _PACK_CACHE.get(key)
    if hit is not None and all(ref() is t for ref, t in zip(hit[0], srcs)):
        return hit[1]
    _PACK_CACHE.pop(key, None)
    if len(_PACK_CACHE) >= _PACK_CACHE_MAX:
        _PACK_CACHE.pop(next(iter(_PACK_CACHE)))
    made = make()
    _PACK_CACHE[key] = (tuple(weakref.ref(t) for t in srcs), made)
    return made


def _pack_layout(w16, b32):
    """[C_out, C_in, 3, 3] float16 (C_in = 32 KS), [C_out] float32 -> the packed pair of include/wgsr.h"""
    c_out, c_in = w16.size(0), w16.size(1)
    rows = (c_out + 15) // 16 * 16
    w = torch.zeros(rows, c_in, 9, dtype=torch.float16, device=w16.device)
    w[:c_out] = w16.reshape(c_out, c_in, 9)
    b = torch.zeros(rows, dtype=torch.float32, device=w16.device)
    b[:c_out] = b32
    # [rb, row, ks, lane >> 4, j, tap] -> [rb, tap, ks, lane >> 4, row, j]: lane = 16 (lane >> 4) + row
    w = w.view(rows // 16, 16, c_in // 32, 4, 8, 9).permute(0, 5, 2, 3, 1, 4).contiguous().view(-1)
    return w, b


def _pack_cached(weights, biases, device=None, c_in=None):
    """The packed pair of the convolutions ``weights`` / ``biases`` stacked along
    their output channels, on ``device`` (default: where the first weight
    lies), kept by ``_cached``.  C_in is any positive multiple of 32, the same
    for all of them; ``c_in``: the value it has to have."""
    for w, b in zip(weights, biases):
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.size(1) == 0 or w.size(1) % 32 or \
                w.size(1) != (c_in or weights[0].size(1)) or b.numel() != w.size(0):
            raise ValueError("a convolution must be weight (C_out, C_in, 3, 3) with C_in "
                             f"{f'= {c_in}' if c_in else 'a positive multiple of 32'} and bias (C_out): got "
                             f"{tuple(w.shape)} and {tuple(b.shape)}")
    device = torch.device(device) if device is not None else weights[0].device

    def make():
        w16 = torch.cat([w.detach().to(device, torch.float16) for w in weights])
        b32 = torch.cat([b.detach().to(device, torch.float32).reshape(-1) for b in biases])
        return _pack_layout(w16, b32)
    return _cached(tuple(weights) + tuple(biases), (device,), make)


def pack_conv3x3(weight, bias):
    """A ``Conv2d(128, C_out, 3, padding=1)``'s ``weight`` [C_out, 128, 3, 3]
    and ``bias`` [C_out] in the order the kernel reads them (include/wgsr.h):
    ``(packed_w, packed_b)`` on the weight's device (host or GPU): the layout
    of ``pack_conv3x3_wide`` with KS = 4, for no other C_in.  The pair is kept
    until the parameter is written again."""
    return _pack_cached((weight,), (bias,), c_in=CONV3X3_CIN)


def unpack_conv3x3(packed_w, packed_b, c_out):
    """The inverse of ``pack_conv3x3``: ``(weight [c_out, 128, 3, 3] float16, bias [c_out] float32)``."""
    return unpack_conv3x3_wide(packed_w, packed_b, c_out, CONV3X3_CIN)


class UpdateHeads:
    """The packed parameters of ``UpdateModule.delta`` / ``.weight`` and of
    ``GraphAgg`` up to ``eta``, packed once: ``hidden`` (delta.0 stacked on
    weight.0, 256 rows: both read ``net``, so they run as one launch), ``delta``,
    ``weight`` (the second layers), ``conv1``, ``conv2``, ``eta``; each a
    ``(packed_w, packed_b)`` pair of ``pack_conv3x3``."""
    NAMES = ("delta.0", "delta.2", "weight.0", "weight.2", "agg.conv1", "agg.conv2", "agg.eta.0")

    def __init__(self, hidden, delta, weight, conv1, conv2, eta):
        self.hidden, self.delta, self.weight, self.conv1, self.conv2, self.eta = hidden, delta, weight, conv1, conv2, eta

    @classmethod
    def from_state_dict(cls, sd, prefix="update.", device=None):
        """From the reference modules' ``state_dict`` entries ``<prefix>weight.0/2``,
        ``delta.0/2``, ``agg.conv1``, ``agg.conv2``, ``agg.eta.0`` (``.weight`` /
        ``.bias`` each)."""
        w = {k: sd[f"{prefix}{k}.weight"] for k in cls.NAMES}
        b = {k: sd[f"{prefix}{k}.bias"] for k in cls.NAMES}
        one = lambda k: _pack_cached((w[k],), (b[k],), device, CONV3X3_CIN)  # noqa: E731
        return cls(_pack_cached((w["delta.0"], w["weight.0"]), (b["delta.0"], b["weight.0"]), device, CONV3X3_CIN),
                   one("delta.2"), one("weight.2"), one("agg.conv1"), one("agg.conv2"), one("agg.eta.0"))


def _update_params(params, dev):
    if isinstance(params, UpdateHeads):
        return params
    prefix = "update." if "update.delta.0.weight" in params else ""
    return UpdateHeads.from_state_dict(params, prefix, dev)


def _activation(name, t, channels, dev, n=None, hw=None, not_contiguous=ValueError, dtypes=(torch.float16,)):
    """One activation of the convolution calls: float16 [n, channels, ht, wd] on
    ``dev``, contiguous (a leading batch dimension of 1 is accepted; ``n`` /
    ``hw`` None: any number of entries / any map size), detached."""
    if t.device != dev:
        droid_backends._device_of(**{name: t})
        raise RuntimeError(f"{name}: expected a tensor on {dev}, got {t.device}")
    if t.dtype not in dtypes:
        if len(dtypes) > 1:
            raise NotImplementedError(f"{name} must be float32 or float16, got {t.dtype}")
        raise NotImplementedError(f"{name}: only float16 activations are built (the tracker's autocast), got "
                                  f"{t.dtype}")
    if t.dim() == 5 and t.size(0) == 1:
        t = t[0]
    if t.dim() != 4 or t.size(1) != channels or (hw is not None and tuple(t.shape[2:]) != hw) or \
            (n is not None and t.size(0) != n):
        want = ("n" if n is None else n, channels) + (("ht", "wd") if hw is None else hw)
        raise ValueError(f"{name} must be ({', '.join(map(str, want))}): got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise not_contiguous(f"{name} must be contiguous")
    return t.detach()


def _conv_net(who, net):
    """the checks update_heads / graph_agg / conv3x3_relu share: (device, net [n, 128, ht, wd])"""
    _inference_only(who, net=net)
    dev = droid_backends._device_of(net=net)
    return dev, _activation("net", net, CONV3X3_CIN, dev, not_contiguous=RuntimeError)  # (CHECK_CONTIGUOUS's type)


def _packed_pair(name, pair, dev, rows, c_in=CONV3X3_CIN):
    """``pair`` = (packed_w, packed_b) of ``rows`` rows of ``c_in`` input channels on ``dev``"""
    w, b = pair
    droid_backends._device_of(**{name: w, name + "_bias": b})
    if w.device != dev:
        raise RuntimeError(f"{name}: expected a tensor on {dev}, got {w.device}")
    if w.dtype != torch.float16 or b.dtype != torch.float32 or b.numel() != rows or \
            w.numel() != rows * c_in * 9 or not w.is_contiguous() or not b.is_contiguous():
        raise ValueError(f"{name}: not a packed pair of {rows} rows of {c_in} input channels (pack_conv3x3_wide)")
    return w, b


def _out_buffer(name, out, shape, dtype, dev):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}")
    return out


def conv3x3_relu(x, packed, out=None):
    """``relu(conv2d(x, weight, bias, padding=1))`` for ``x`` [n, 128, ht, wd]
    float16 and ``packed = pack_conv3x3(weight, bias)`` with C_out a multiple of
    128: float16 [n, C_out, ht, wd], fp32 MFMA accumulation, one rounding --
    the convolution of this file on its own."""
    dev, x = _conv_net("conv3x3_relu", x)
    rows = packed[1].numel()
    w, b = _packed_pair("packed", packed, dev, rows)
    n, _, ht, wd = x.shape
    out = _out_buffer("out", out, (n, rows, ht, wd), torch.float16, dev)
    if out.numel():
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wgsr_droid_conv3x3_relu(x.data_ptr(), w.data_ptr(), b.data_ptr(), rows,
                                                           out.data_ptr(), n, ht, wd, _lib.stream_handle(dev)))
    return out


def update_heads(net, params, out=None):
    """``UpdateModule``'s ``delta`` and ``weight`` heads on the GRU's output
    (droid_net.py:141-145): ``net`` [n, 128, ht, wd] float16 (a leading batch
    dimension of 1 is accepted) -> ``(delta, weight)``, each [n, ht, wd, 2]
    float32, the permuted form the reference returns.  ``params``: an
    ``UpdateHeads`` or the modules' ``state_dict``.  Both hidden convolutions
    run as one 256-row launch whose float16 result (autocast's rounding point)
    the two second layers read; delta and sigmoid(weight) are fp32 values never
    rounded to float16.  No host read; capturable in a graph.  ``out``: the
    pair of buffers to write instead of new ones."""
    dev, net = _conv_net("update_heads", net)
    p = _update_params(params, dev)
    hw, hb = _packed_pair("hidden", p.hidden, dev, 2 * CONV3X3_CIN)
    dw, db = _packed_pair("delta", p.delta, dev, 16)
    ww, wb = _packed_pair("weight", p.weight, dev, 16)
    n, _, ht, wd = net.shape
    delta = _out_buffer("delta", out[0] if out else None, (n, ht, wd, 2), torch.float32, dev)
    weight = _out_buffer("weight", out[1] if out else None, (n, ht, wd, 2), torch.float32, dev)
    if delta.numel():
        hidden = torch.empty(n, 2 * CONV3X3_CIN, ht, wd, dtype=torch.float16, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wgsr_droid_update_heads(
                net.data_ptr(), hw.data_ptr(), hb.data_ptr(), dw.data_ptr(), db.data_ptr(), ww.data_ptr(),
                wb.data_ptr(), hidden.data_ptr(), delta.data_ptr(), weight.data_ptr(), n, ht, wd,
                _lib.stream_handle(dev)))
    return delta, weight


def graph_agg(net, ii, params, ix=None, num_groups=None, check=True, out=None):
    """``GraphAgg.forward`` up to ``eta`` and the input of ``upmask``
    (droid_net.py:65-77): ``net`` [n, 128, ht, wd] float16 (a leading batch
    dimension of 1 is accepted), ``ii`` [n] the source frame of each edge ->
    ``(eta, feat)``: ``eta`` [G, ht, wd] float32 (0.01 softplus, never rounded
    to float16), ``feat`` [G, 128, ht, wd] float16, which
    ``upsample_from_features`` takes unchanged:

        eta, feat = graph_agg(net, ii, params)
        upsample_from_features(video.disps, video.disps_up, torch.unique(ii), feat, upmask_weight, upmask_bias)

    replaces ``GraphAgg.forward`` + ``DepthVideo.upsample``.  With ``ix`` /
    ``num_groups`` left out the groups are ``torch.unique(ii, sorted=True,
    return_inverse=True)`` as in the reference, which is one host read (the
    number of groups).  With both given (``ix`` [n] int64 on the device, each in
    [0, num_groups); ``ii`` is then unused) there is no host read; the kernel
    validates ``ix`` and ``check`` reads the status word back and raises
    ``RuntimeError`` (nothing was written); ``check=False`` skips that read and
    the call can be captured in a graph.  The mean over a group's edges is an
    fp32 sum in ascending edge order by one lane per element (bit-identical
    between runs), rounded to float16 once; a group without an edge gives the
    mean zero, as ``scatter_mean``."""
    dev, net = _conv_net("graph_agg", net)
    p = _update_params(params, dev)
    c1 = _packed_pair("conv1", p.conv1, dev, CONV3X3_CIN)
    c2 = _packed_pair("conv2", p.conv2, dev, CONV3X3_CIN)
    ce = _packed_pair("eta", p.eta, dev, 16)
    n, _, ht, wd = net.shape
    if (ix is None) != (num_groups is None):
        raise ValueError("ix and num_groups are given together or not at all")
    if ix is None:
        ii = torch.as_tensor(ii).to(dev).reshape(-1)
        uniq, ix = torch.unique(ii, sorted=True, return_inverse=True)
        num_groups = uniq.numel()
    ix = _upsample_index(ix, dev)
    G = int(num_groups)
    if ix.numel() != n:
        raise ValueError(f"{ix.numel()} group indices for the {n} edges of net")
    if G < 0 or (G == 0 and n):
        raise ValueError(f"num_groups = {G} for {n} edges")
    eta = _out_buffer("eta", out[0] if out else None, (G, ht, wd), torch.float32, dev)
    feat = _out_buffer("feat", out[1] if out else None, (G, CONV3X3_CIN, ht, wd), torch.float16, dev)
    if not eta.numel():
        return eta, feat
    mean = torch.empty(G, CONV3X3_CIN, ht, wd, dtype=torch.float16, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().wgsr_droid_graph_agg(
            net.data_ptr(), ix.data_ptr(), n, G, c1[0].data_ptr(), c1[1].data_ptr(), c2[0].data_ptr(),
            c2[1].data_ptr(), ce[0].data_ptr(), ce[1].data_ptr(), mean.data_ptr(), feat.data_ptr(), eta.data_ptr(),
            ht, wd, status.data_ptr(), _lib.stream_handle(dev)))
    if check:
        _raise_status("graph_agg", status, GRAPH_AGG_STATUS)
    return eta, feat


# ---------------------------------------------------------------------------
# The update operator's ConvGRU (csrc/droid_gru.hip)
# ---------------------------------------------------------------------------
GRU_CIN = 3 * CONV3X3_CIN + CONV3X3_CIN // 2   # net, inp, corr [128 each], flow [64]
GRU_GLO_CHUNK = 128                            # kGrGloPix: pixels of one partial sum of the glo term
GRU_STATUS = {1: "an entry of inp_ix is outside the frames of inp (WGSR_GRU_BAD_IX)"}


def pack_conv3x3_wide(weight, bias):
    """A ``Conv2d(C_in, C_out, 3, padding=1)``'s ``weight`` [C_out, C_in, 3, 3]
    (C_in a multiple of 32) and ``bias`` [C_out] in the order the kernels read
    them (include/wgsr.h): ``(packed_w, packed_b)`` on the weight's device (host
    or GPU).  With KS = C_in / 32 and R = ceil(C_out / 16), ``packed_w`` is
    float16 [R * 9 * KS * 64 * 8],

        packed_w[(((rb 9 + tap) KS + ks) 64 + lane) 8 + j]
            = weight[16 rb + (lane & 15), 32 ks + 8 (lane >> 4) + j, tap // 3, tap % 3]

    (weights rounded to float16 once, zeros in the rows past C_out) and
    ``packed_b`` float32 [16 R], zero past C_out.  The pair is kept until the
    parameter is written again."""
    return _pack_cached((weight,), (bias,))


def unpack_conv3x3_wide(packed_w, packed_b, c_out, c_in):
    """The inverse of ``pack_conv3x3_wide``: ``(weight [c_out, c_in, 3, 3] float16, bias [c_out] float32)``."""
    rows = packed_b.numel()
    if c_in <= 0 or c_in % 32 or rows % 16 or packed_w.numel() != rows * c_in * 9 or not 0 < c_out <= rows:
        raise ValueError(f"not a packed pair of {c_out} rows of {c_in} input channels: {packed_w.numel()} weights, "
                         f"{rows} biases")
    w = packed_w.view(rows // 16, 9, c_in // 32, 4, 16, 8).permute(0, 4, 2, 3, 5, 1).reshape(rows, c_in, 3, 3)
    return w[:c_out].contiguous(), packed_b[:c_out].clone()


def _gru_glo_cached(weights, biases, device):
    """``(glo_w, glo_b)`` of include/wgsr.h from ``weights`` = (w, convz_glo,
    convr_glo, convq_glo) and ``biases`` = (w, convz, convr, convq, convz_glo,
    convr_glo, convq_glo), kept by ``_cached``."""
    for w in weights:
        if w.numel() != CONV3X3_CIN * CONV3X3_CIN or w.size(0) != CONV3X3_CIN:
            raise ValueError(f"a glo convolution must be weight ({CONV3X3_CIN}, {CONV3X3_CIN}, 1, 1): got "
                             f"{tuple(w.shape)}")
    for b in biases:
        if b.numel() != CONV3X3_CIN:
            raise ValueError(f"a bias of the GRU must hold {CONV3X3_CIN} values: got {tuple(b.shape)}")

    def make():
        w16 = [w.detach().to(device, torch.float16).reshape(CONV3X3_CIN, CONV3X3_CIN) for w in weights]
        # w as one tap: [rb, row, ks, lane >> 4, j] -> [rb, ks, lane >> 4, row, j]
        first = w16[0].view(8, 16, 4, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)
        glo_w = torch.cat([first] + [w.reshape(-1) for w in w16[1:]])
        return glo_w, torch.cat([b.detach().to(device, torch.float32).reshape(-1) for b in biases])
    return _cached(tuple(weights) + tuple(biases), (device, "glo"), make)


class UpdateGRU:
    """The packed parameters of ``UpdateModule.gru`` (gru.py:19-32), packed
    once: ``zr`` (convz stacked on convr, 256 rows: both read [net, inp, corr,
    flow], so they run as one launch) and ``q`` (convq), each a ``(packed_w,
    packed_b)`` pair of ``pack_conv3x3_wide`` with C_in = 448; ``glo_w`` (w packed
    as one tap, then convz_glo, convr_glo, convq_glo as they lie) and ``glo_b``
    (the biases of w, of convz, convr, convq and of the three glo convolutions:
    float32 [896], the biases the kernels read), the layout of include/wgsr.h."""
    NAMES = ("convz", "convr", "convq", "w", "convz_glo", "convr_glo", "convq_glo")

    def __init__(self, zr, q, glo_w, glo_b):
        self.zr, self.q, self.glo_w, self.glo_b = zr, q, glo_w, glo_b

    @classmethod
    def from_state_dict(cls, sd, prefix="update.gru.", device=None):
        """From the reference module's ``state_dict`` entries ``<prefix>convz``,
        ``convr``, ``convq``, ``w``, ``convz_glo``, ``convr_glo``, ``convq_glo``
        (``.weight`` / ``.bias`` each)."""
        w = {k: sd[f"{prefix}{k}.weight"] for k in cls.NAMES}
        b = {k: sd[f"{prefix}{k}.bias"] for k in cls.NAMES}
        device = torch.device(device) if device is not None else w["convz"].device
        for k in ("convz", "convr", "convq"):
            if w[k].dim() != 4 or w[k].size(1) != GRU_CIN or w[k].size(0) != CONV3X3_CIN:
                raise ValueError(f"{k} must be weight ({CONV3X3_CIN}, {GRU_CIN}, 3, 3): got {tuple(w[k].shape)}")
        glo = ("w", "convz_glo", "convr_glo", "convq_glo")
        glo_w, glo_b = _gru_glo_cached([w[k] for k in glo],
                                       [b[k] for k in ("w", "convz", "convr", "convq") + glo[1:]], device)
        return cls(_pack_cached((w["convz"], w["convr"]), (b["convz"], b["convr"]), device),
                   _pack_cached((w["convq"],), (b["convq"],), device), glo_w, glo_b)


def _gru_params(params, dev):
    if isinstance(params, UpdateGRU):
        return params
    for prefix in ("update.gru.", "gru.", ""):
        if f"{prefix}convz.weight" in params:
            return UpdateGRU.from_state_dict(params, prefix, dev)
    raise ValueError("params holds no convz.weight under update.gru., gru. or no prefix")


def _gru_overlap(a, b):
    la, lb = a.data_ptr(), b.data_ptr()
    return a.numel() and b.numel() and la < lb + b.numel() * b.element_size() and \
        lb < la + a.numel() * a.element_size()


def conv_gru(net, inp, corr, flow, params, inp_ix=None, check=True, out=None, return_intermediates=False,
             scratch=None):
    """``ConvGRU.forward`` as the update operator calls it (droid_net.py:138,
    ``self.gru(net, inp, corr, flow)``; gru.py:34-48): ``net``, ``corr`` [n, 128,
    ht, wd] and ``flow`` [n, 64, ht, wd] float16 (a leading batch dimension of 1
    is accepted) -> ``net'`` float16 [n, 128, ht, wd].  ``inp`` is [n, 128, ht,
    wd], or with ``inp_ix`` [n] (int64) the per-frame buffer [F, 128, ht, wd] of
    which edge e reads frame ``inp_ix[e]``, no gathered copy (``video.inps`` and
    ``iis`` in ``update_lowmem``).  ``params``: an ``UpdateGRU`` or the
    ``state_dict``.  Four launches: the glo term (two; ``gbias`` [n, 384] float32,
    the convolutions' biases added), z and r * net (one 256-row convolution over
    the four sources), then q and the blend.  fp32 inside a launch; z, r * net
    and net' are the only float16 roundings.  ``return_intermediates``:
    ``(net', {"gbias", "z", "rnet"})``.  The kernels validate ``inp_ix`` on the
    device; ``check`` reads the status word back and raises ``RuntimeError``
    (nothing was written); ``check=False`` skips that read: no synchronisation,
    and the call can be captured in a graph (``inp_ix`` then has to be a device
    tensor already).  ``out`` / ``scratch``: the buffer for ``net'`` and the
    triple ``(gbias, z, rnet)`` to write instead of new ones (a fourth entry:
    the glo term's partial sums, float32 [n, ceil(ht wd / 128), 128])."""
    _inference_only("conv_gru", net=net, inp=inp, corr=corr, flow=flow)
    dev = droid_backends._device_of(net=net, inp=inp, corr=corr, flow=flow)
    net = _activation("net", net, CONV3X3_CIN, dev)
    n, _, ht, wd = net.shape
    corr = _activation("corr", corr, CONV3X3_CIN, dev, n, (ht, wd))
    flow = _activation("flow", flow, CONV3X3_CIN // 2, dev, n, (ht, wd))
    inp = _activation("inp", inp, CONV3X3_CIN, dev, None if inp_ix is not None else n, (ht, wd))
    frames = 0
    if inp_ix is not None:
        inp_ix = _upsample_index(inp_ix, dev)
        frames = inp.size(0)
        if inp_ix.numel() != n:
            raise ValueError(f"{inp_ix.numel()} entries of inp_ix for the {n} edges of net")
        if n and not frames:
            raise ValueError("inp holds no frame")
    p = _gru_params(params, dev)
    _packed_pair("zr", p.zr, dev, 2 * CONV3X3_CIN, GRU_CIN)  # (the kernels read the biases from glo_b)
    _packed_pair("q", p.q, dev, CONV3X3_CIN, GRU_CIN)
    if p.glo_w.device != dev or p.glo_b.device != dev:
        raise RuntimeError(f"glo: expected tensors on {dev}, got {p.glo_w.device} and {p.glo_b.device}")
    if p.glo_w.dtype != torch.float16 or p.glo_w.numel() != 4 * CONV3X3_CIN ** 2 or p.glo_b.dtype != torch.float32 \
            or p.glo_b.numel() != 7 * CONV3X3_CIN or not p.glo_w.is_contiguous() or not p.glo_b.is_contiguous():
        raise ValueError("glo_w / glo_b: not the packed glo parameters (UpdateGRU.from_state_dict)")
    out = _out_buffer("out", out, (n, CONV3X3_CIN, ht, wd), torch.float16, dev)
    for name, t in (("net", net), ("inp", inp), ("corr", corr), ("flow", flow)):
        if _gru_overlap(out, t):
            raise ValueError(f"out must not overlap {name}")
    gbias = _out_buffer("gbias", scratch[0] if scratch else None, (n, 3 * CONV3X3_CIN), torch.float32, dev)
    z = _out_buffer("z", scratch[1] if scratch else None, out.shape, torch.float16, dev)
    rnet = _out_buffer("rnet", scratch[2] if scratch else None, out.shape, torch.float16, dev)
    part = _out_buffer("glo_part", scratch[3] if scratch and len(scratch) > 3 else None,
                       (n, (ht * wd + GRU_GLO_CHUNK - 1) // GRU_GLO_CHUNK, CONV3X3_CIN), torch.float32, dev)
    if out.numel():
        status = torch.empty(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wgsr_droid_gru(
                net.data_ptr(), inp.data_ptr(), _lib.ptr(inp_ix), frames, corr.data_ptr(), flow.data_ptr(),
                p.glo_w.data_ptr(), p.glo_b.data_ptr(), p.zr[0].data_ptr(), p.q[0].data_ptr(), gbias.data_ptr(),
                part.data_ptr(), z.data_ptr(), rnet.data_ptr(), out.data_ptr(), n, ht, wd, status.data_ptr(),
                _lib.stream_handle(dev)))
        if check and inp_ix is not None:
            _raise_status("conv_gru", status, GRU_STATUS)
    if return_intermediates:
        return out, {"gbias": gbias, "z": z, "rnet": rnet}
    return out


# ---------------------------------------------------------------------------
# The update operator's corr and flow encoders (csrc/droid_encoders.hip) and
# the whole operator
# ---------------------------------------------------------------------------
CORR_PLANES = 196            # 4 levels x 7 x 7: what corr_lookup / AltCorrBlock write
FLOW_PLANES = 4
ENC_HIDDEN = CONV3X3_CIN     # channels of both encoders' hidden layer
ENC_KS = 7                   # K-steps of a first layer: 196 products padded to 224


def _pack_first_cached(weight, bias, shape, device, layout):
    """The packed pair of a first layer (``layout``: [128, *shape[1:]] float16 ->
    [rb, row, ks, lane >> 4, j] with zeros in the padded K slots), kept by ``_cached``."""
    if tuple(weight.shape) != shape or bias.numel() != shape[0]:
        raise ValueError(f"a first layer must be weight {shape} and bias ({shape[0]}): got {tuple(weight.shape)} and "
                         f"{tuple(bias.shape)}")
    device = torch.device(device) if device is not None else weight.device

    def make():
        w = layout(weight.detach().to(device, torch.float16))
        # [rb, row, ks, lane >> 4, j] -> [rb, ks, lane >> 4, row, j]: lane = 16 (lane >> 4) + row
        w = w.reshape(ENC_HIDDEN // 16, 16, ENC_KS, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)
        return w, bias.detach().to(device, torch.float32).reshape(-1).contiguous()
    return _cached((weight, bias), (device, "first", shape), make)


def _unpack_first(packed_w, packed_b):
    if packed_w.numel() != ENC_HIDDEN * 32 * ENC_KS or packed_b.numel() != ENC_HIDDEN:
        raise ValueError(f"not a packed first layer: {packed_w.numel()} weights, {packed_b.numel()} biases")
    return packed_w.view(ENC_HIDDEN // 16, ENC_KS, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(ENC_HIDDEN, 32 * ENC_KS)


def pack_conv1x1_196(weight, bias, device=None):
    """``corr_encoder.0``, a ``Conv2d(196, 128, 1)``: ``weight`` [128, 196, 1, 1]
    and ``bias`` [128] in the order the kernel reads them (include/wgsr.h):
    ``packed_w`` float16 [8 * 7 * 64 * 8],

        packed_w[((rb 7 + ks) 64 + lane) 8 + j] = weight[16 rb + (lane & 15), 32 ks + 8 (lane >> 4) + j]

    with zeros past channel 195 (K = 224), and ``packed_b`` float32 [128]."""
    def layout(w16):
        w = torch.zeros(ENC_HIDDEN, 32 * ENC_KS, dtype=torch.float16, device=w16.device)
        w[:, :CORR_PLANES] = w16.reshape(ENC_HIDDEN, CORR_PLANES)
        return w
    return _pack_first_cached(weight, bias, (ENC_HIDDEN, CORR_PLANES, 1, 1), device, layout)


def unpack_conv1x1_196(packed_w, packed_b):
    """The inverse of ``pack_conv1x1_196``: ``(weight [128, 196, 1, 1] float16, bias [128] float32)``."""
    w = _unpack_first(packed_w, packed_b)
    return w[:, :CORR_PLANES].reshape(ENC_HIDDEN, CORR_PLANES, 1, 1).contiguous(), packed_b.clone()


def pack_conv7x7_4(weight, bias, device=None):
    """``flow_encoder.0``, a ``Conv2d(4, 128, 7, padding=3)``: ``weight`` [128, 4,
    7, 7] and ``bias`` [128] in the order the kernel reads them (include/wgsr.h):
    K index 32 ky + 4 kx + ci with kx = 7 a zero pad, so that one K-step is one
    kernel row: ``packed_w`` float16 [8 * 7 * 64 * 8],

        packed_w[((rb 7 + ks) 64 + lane) 8 + j] = weight[16 rb + (lane & 15), j & 3, ks, 2 (lane >> 4) + (j >> 2)]

    and ``packed_b`` float32 [128]."""
    def layout(w16):
        w = torch.zeros(ENC_HIDDEN, 7, 8, FLOW_PLANES, dtype=torch.float16, device=w16.device)
        w[:, :, :7] = w16.permute(0, 2, 3, 1)  # [row, ky, kx, ci]
        return w
    return _pack_first_cached(weight, bias, (ENC_HIDDEN, FLOW_PLANES, 7, 7), device, layout)


def unpack_conv7x7_4(packed_w, packed_b):
    """The inverse of ``pack_conv7x7_4``: ``(weight [128, 4, 7, 7] float16, bias [128] float32)``."""
    w = _unpack_first(packed_w, packed_b).view(ENC_HIDDEN, 7, 8, FLOW_PLANES)
    return w[:, :, :7].permute(0, 3, 1, 2).contiguous(), packed_b.clone()


class UpdateEncoders:
    """The packed parameters of ``UpdateModule.corr_encoder`` / ``.flow_encoder``,
    packed once: ``corr1`` (``pack_conv1x1_196``), ``corr2`` (``pack_conv3x3``, 128
    rows), ``flow1`` (``pack_conv7x7_4``), ``flow2`` (``pack_conv3x3``, 64 rows);
    each a ``(packed_w, packed_b)`` pair."""
    NAMES = ("corr_encoder.0", "corr_encoder.2", "flow_encoder.0", "flow_encoder.2")

    def __init__(self, corr1, corr2, flow1, flow2):
        self.corr1, self.corr2, self.flow1, self.flow2 = corr1, corr2, flow1, flow2

    @classmethod
    def from_state_dict(cls, sd, prefix="update.", device=None):
        """From the reference module's ``state_dict`` entries ``<prefix>corr_encoder.0/2``
        and ``flow_encoder.0/2`` (``.weight`` / ``.bias`` each)."""
        w = {k: sd[f"{prefix}{k}.weight"] for k in cls.NAMES}
        b = {k: sd[f"{prefix}{k}.bias"] for k in cls.NAMES}
        for k, rows in (("corr_encoder.2", CONV3X3_CIN), ("flow_encoder.2", CONV3X3_CIN // 2)):
            if w[k].dim() != 4 or w[k].size(0) != rows:
                raise ValueError(f"{k} must be weight ({rows}, {CONV3X3_CIN}, 3, 3): got {tuple(w[k].shape)}")
        return cls(pack_conv1x1_196(w["corr_encoder.0"], b["corr_encoder.0"], device),
                   _pack_cached((w["corr_encoder.2"],), (b["corr_encoder.2"],), device, CONV3X3_CIN),
                   pack_conv7x7_4(w["flow_encoder.0"], b["flow_encoder.0"], device),
                   _pack_cached((w["flow_encoder.2"],), (b["flow_encoder.2"],), device, CONV3X3_CIN))


def _encoder_params(params, dev):
    if isinstance(params, UpdateEncoders):
        return params
    prefix = "update." if "update.corr_encoder.0.weight" in params else ""
    return UpdateEncoders.from_state_dict(params, prefix, dev)


def _first_pair(name, pair, dev):
    w, b = pair
    droid_backends._device_of(**{name: w, name + "_bias": b})
    if w.device != dev:
        raise RuntimeError(f"{name}: expected a tensor on {dev}, got {w.device}")
    if w.dtype != torch.float16 or b.dtype != torch.float32 or b.numel() != ENC_HIDDEN or \
            w.numel() != ENC_HIDDEN * 32 * ENC_KS or not w.is_contiguous() or not b.is_contiguous():
        raise ValueError(f"{name}: not a packed first layer (pack_conv1x1_196 / pack_conv7x7_4)")
    return w, b


def _encoder_out(name, out, shape, dev, src):
    out = _out_buffer("out", out, shape, torch.float16, dev)
    if _gru_overlap(out, src):
        raise ValueError(f"out must not overlap {name}")
    return out


def corr_encoder(corr, params, out=None):
    """``UpdateModule.corr_encoder`` (droid_net.py:88-93, 136): ``corr`` [n, 196,
    ht, wd] float16, what ``corr_lookup`` / ``CorrBlock`` / ``AltCorrBlock``
    return (a leading batch dimension of 1 is accepted) -> float16 [n, 128, ht,
    wd], the ``corr`` argument of ``conv_gru``.  ``params``: an
    ``UpdateEncoders`` or the modules' ``state_dict``.
    One launch: the 1 x 1 convolution on each tile with its halo, its float16
    result (autocast's rounding point, zero outside the map) kept in LDS, the
    3 x 3 convolution on that; fp32 accumulation, one rounding of the output.
    No host read; capturable in a graph.  ``out``: the buffer to write instead
    of a new one."""
    _inference_only("corr_encoder", corr=corr)
    dev = droid_backends._device_of(corr=corr)
    corr = _activation("corr", corr, CORR_PLANES, dev)
    p = _encoder_params(params, dev)
    w1, b1 = _first_pair("corr1", p.corr1, dev)
    w2, b2 = _packed_pair("corr2", p.corr2, dev, CONV3X3_CIN)
    n, _, ht, wd = corr.shape
    out = _encoder_out("corr", out, (n, CONV3X3_CIN, ht, wd), dev, corr)
    if out.numel():
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wgsr_droid_corr_encoder(
                corr.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.data_ptr(), n, ht, wd,
                _lib.stream_handle(dev)))
    return out


def flow_encoder(flow, params, out=None):
    """``UpdateModule.flow_encoder`` (droid_net.py:95-100, 137): ``flow`` [n, 4,
    ht, wd] float32 (what factor_graph.py passes as ``motn``) or float16 (a
    leading batch dimension of 1 is accepted) -> float16 [n, 64, ht, wd], the
    ``flow`` argument of ``conv_gru``.  A float32 input is rounded to float16
    (round to nearest even) as the kernel reads it, which is autocast's cast:
    both dtypes of the same values give the same bits.  One launch, as
    ``corr_encoder``: the 7 x 7 convolution on each tile with its halo, its
    float16 result kept in LDS (zero outside the map), the 3 x 3 convolution on
    that.  ``params`` and ``out`` as there."""
    _inference_only("flow_encoder", flow=flow)
    dev = droid_backends._device_of(flow=flow)
    flow = _activation("flow", flow, FLOW_PLANES, dev, dtypes=tuple(droid_backends._DTYPE_TAG))
    p = _encoder_params(params, dev)
    w1, b1 = _first_pair("flow1", p.flow1, dev)
    w2, b2 = _packed_pair("flow2", p.flow2, dev, CONV3X3_CIN // 2)
    n, _, ht, wd = flow.shape
    out = _encoder_out("flow", out, (n, CONV3X3_CIN // 2, ht, wd), dev, flow)
    if out.numel():
        with torch.cuda.device(dev):
            _lib.check(_lib.load().wgsr_droid_flow_encoder(
                flow.data_ptr(), droid_backends._DTYPE_TAG[flow.dtype], w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                b2.data_ptr(), out.data_ptr(), n, ht, wd, _lib.stream_handle(dev)))
    return out


class UpdateOperator:
    """The packed parameters of the whole ``UpdateModule``: ``encoders``
    (``UpdateEncoders``), ``gru`` (``UpdateGRU``), ``heads`` (``UpdateHeads``)."""

    def __init__(self, encoders, gru, heads):
        self.encoders, self.gru, self.heads = encoders, gru, heads

    @classmethod
    def from_state_dict(cls, sd, prefix="update.", device=None):
        """From the reference's ``state_dict`` entries under ``prefix`` (``DroidNet``'s: "update.")."""
        return cls(UpdateEncoders.from_state_dict(sd, prefix, device),
                   UpdateGRU.from_state_dict(sd, prefix + "gru.", device),
                   UpdateHeads.from_state_dict(sd, prefix, device))


def update_operator(net, inp, corr, flow=None, ii=None, params=None, inp_ix=None, num_groups=None, check=True,
                    out=None):
    """``UpdateModule.forward`` (droid_net.py:120-153) as one call: ``net`` [n,
    128, ht, wd] float16, ``inp`` as ``conv_gru`` takes it (with ``inp_ix`` the
    per-frame buffer), ``corr`` [n, 196, ht, wd] float16, ``flow`` [n, 4, ht, wd]
    float32 or float16, None: zeros, as in the reference (the motion filter)
    -> ``(net', delta, weight)``, or with ``ii`` [n] ``(net', delta, weight, eta,
    feat)``: ``net'`` float16 [n, 128, ht, wd], ``delta`` / ``weight`` float32 [n,
    ht, wd, 2], ``eta`` float32 [G, ht, wd], ``feat`` float16 [G, 128, ht, wd],
    which ``upsample_from_features`` takes in place of the reference's upmask.
    The composition ``corr_encoder``, ``flow_encoder`` -> ``conv_gru`` ->
    ``update_heads`` -> ``graph_agg``, bit-identical to those calls.  ``params``:
    an ``UpdateOperator`` or the ``state_dict`` of ``UpdateModule`` /
    ``DroidNet``.  With ``num_groups`` given, ``ii`` holds each edge's group in
    [0, num_groups) already (``graph_agg``'s ``ix``) and no ``torch.unique`` runs.
    ``check=False`` skips the reads of the status words: with ``num_groups`` (or
    without ``ii``) the whole call then makes no host read and can be captured in
    a graph.  ``out``: the buffers of the returned tuple to write instead of new
    ones; a status error leaves those of its call and of the later calls
    untouched."""
    if params is None:
        raise ValueError("params: an UpdateOperator or the state_dict of the update module")
    if not isinstance(params, UpdateOperator):
        prefix = "update." if "update.corr_encoder.0.weight" in params else ""
        params = UpdateOperator.from_state_dict(params, prefix, net.device)
    if flow is None:
        lead = net.shape[:-3]
        flow = torch.zeros(*lead, FLOW_PLANES, *net.shape[-2:], dtype=torch.float32, device=net.device)
    hw = tuple(net.shape[-2:])
    for name, t in (("corr", corr), ("flow", flow)):
        if tuple(t.shape[-2:]) != hw or t.shape[:-3] != net.shape[:-3]:
            raise ValueError(f"{name} must hold the {tuple(net.shape[:-3])} maps of {hw[0]} x {hw[1]} of net: got "
                             f"{tuple(t.shape)}")
    corr = corr_encoder(corr, params.encoders)
    flow = flow_encoder(flow, params.encoders)
    if out is not None and len(out) != (3 if ii is None else 5):
        raise ValueError(f"out must hold the {3 if ii is None else 5} buffers of the returned tuple")
    net = conv_gru(net, inp, corr, flow, params.gru, inp_ix=inp_ix, check=check, out=out[0] if out else None)
    delta, weight = update_heads(net, params.heads, out=out[1:3] if out else None)
    if ii is None:
        return net, delta, weight
    if num_groups is None:
        eta, feat = graph_agg(net, ii, params.heads, out=out[3:] if out else None)
    else:
        eta, feat = graph_agg(net, None, params.heads, ix=ii, num_groups=num_groups, check=check,
                              out=out[3:] if out else None)
    return net, delta, weight, eta, feat


# ---------------------------------------------------------------------------
# The feature and context encoders, DroidNet.fnet / .cnet (csrc/droid_basic_encoder.hip)
# ---------------------------------------------------------------------------
BE_DIMS = (32, 64, 128)      # channels of the stem / layer1, layer2, layer3
BE_STEM_KS = 5               # K-steps of the stem: 147 products padded to 160
BE_STEM_K = 147
BE_OUT = {"instance": 128, "none": 256}   # the head's rows: fnet; cnet (net stacked on inp)
BE_LAYERS = ("layer1.0", "layer1.1", "layer2.0", "layer2.1", "layer3.0", "layer3.1")
# the launches after the stem: the convolution, the raw map it normalises and reads, the second term (a block output
# X: form B; a downsample's raw output Rd: form C; None: form A), the side output, C_in, stride, the raw map it writes
BE_LAUNCHES = (("layer1.0.conv1", "R0", None, "X0", 32, 1, "R1"), ("layer1.0.conv2", "R1", None, None, 32, 1, "R2"),
               ("layer1.1.conv1", "R2", "X0", "X1", 32, 1, "R3"), ("layer1.1.conv2", "R3", None, None, 32, 1, "R4"),
               ("layer2.0.conv1", "R4", "X1", None, 32, 2, "R5"), ("layer2.0.conv2", "R5", None, None, 64, 1, "R6"),
               ("layer2.1.conv1", "R6", "Rd5", "X3", 64, 1, "R7"), ("layer2.1.conv2", "R7", None, None, 64, 1, "R8"),
               ("layer3.0.conv1", "R8", "X3", None, 64, 2, "R9"), ("layer3.0.conv2", "R9", None, None, 128, 1, "R10"),
               ("layer3.1.conv1", "R10", "Rd9", "X5", 128, 1, "R11"),
               ("layer3.1.conv2", "R11", None, None, 128, 1, "R12"))


def pack_stem7x7(weight, bias, device=None):
    """The encoders' first layer, a ``Conv2d(3, 32, 7, stride=2, padding=3)``:
    ``weight`` [32, 3, 7, 7] and ``bias`` [32] in the order the kernel reads them
    (include/wgsr.h): product k = 21 ky + 3 kx + ci, 147 of them padded to 160 =
    5 K-steps with zero weights, ``packed_w`` float16 [2 * 5 * 64 * 8],

        packed_w[((rb 5 + ks) 64 + lane) 8 + j] = weight[16 rb + (lane & 15), ci, ky, kx],
            21 ky + 3 kx + ci = 32 ks + 8 (lane >> 4) + j

    and ``packed_b`` float32 [32].  The pair is kept until the parameter is
    written again."""
    _stem_check(weight, bias)
    device = torch.device(device) if device is not None else weight.device
    return _cached((weight, bias), (device, "stem"), lambda: _stem_layout(weight, bias, device))


def _stem_check(weight, bias):
    shape = (BE_DIMS[0], 3, 7, 7)
    if tuple(weight.shape) != shape or bias.numel() != shape[0]:
        raise ValueError(f"the stem must be weight {shape} and bias ({shape[0]}): got {tuple(weight.shape)} and "
                         f"{tuple(bias.shape)}")


def _stem_layout(weight, bias, device):
    rows = BE_DIMS[0]
    w = torch.zeros(rows, 32 * BE_STEM_KS, dtype=torch.float16, device=device)
    w[:, :BE_STEM_K] = weight.detach().to(device, torch.float16).permute(0, 2, 3, 1).reshape(rows, BE_STEM_K)
    # [rb, row, ks, lane >> 4, j] -> [rb, ks, lane >> 4, row, j]
    w = w.view(rows // 16, 16, BE_STEM_KS, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)
    return w, bias.detach().to(device, torch.float32).reshape(-1).contiguous()


def unpack_stem7x7(packed_w, packed_b):
    """The inverse of ``pack_stem7x7``: ``(weight [32, 3, 7, 7] float16, bias [32] float32)``."""
    rows = BE_DIMS[0]
    if packed_w.numel() != rows * 32 * BE_STEM_KS or packed_b.numel() != rows:
        raise ValueError(f"not a packed stem: {packed_w.numel()} weights, {packed_b.numel()} biases")
    w = packed_w.view(rows // 16, BE_STEM_KS, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(rows, 32 * BE_STEM_KS)
    return w[:, :BE_STEM_K].reshape(rows, 7, 7, 3).permute(0, 3, 1, 2).contiguous(), packed_b.clone()


def pack_conv1x1(weight, bias, device=None):
    """A ``Conv2d(C_in, C_out, 1)``'s ``weight`` [C_out, C_in, 1, 1] (C_in a multiple
    of 32, C_out of 16) and ``bias`` [C_out] in the order the kernel reads them
    (include/wgsr.h): the layout of ``pack_conv3x3_wide`` with one tap, with KS =
    C_in / 32 ``packed_w`` float16 [C_out / 16 * KS * 64 * 8],

        packed_w[((rb KS + ks) 64 + lane) 8 + j] = weight[16 rb + (lane & 15), 32 ks + 8 (lane >> 4) + j]

    and ``packed_b`` float32 [C_out].  The pair is kept until the parameter is
    written again."""
    _conv1x1_check(weight, bias)
    device = torch.device(device) if device is not None else weight.device
    return _cached((weight, bias), (device, "1x1"), lambda: _conv1x1_layout(weight, bias, device))


def _conv1x1_check(weight, bias):
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1) or weight.size(1) == 0 or weight.size(1) % 32 or \
            weight.size(0) == 0 or weight.size(0) % 16 or bias.numel() != weight.size(0):
        raise ValueError("a 1 x 1 convolution must be weight (C_out, C_in, 1, 1) with C_in a positive multiple of 32, "
                         f"C_out of 16, and bias (C_out): got {tuple(weight.shape)} and {tuple(bias.shape)}")


def _conv1x1_layout(weight, bias, device):
    c_out, c_in = weight.size(0), weight.size(1)
    w = weight.detach().to(device, torch.float16).reshape(c_out // 16, 16, c_in // 32, 4, 8)
    return (w.permute(0, 2, 3, 1, 4).contiguous().view(-1),
            bias.detach().to(device, torch.float32).reshape(-1).contiguous())


def unpack_conv1x1(packed_w, packed_b, c_in):
    """The inverse of ``pack_conv1x1``: ``(weight [C_out, c_in, 1, 1] float16, bias [C_out] float32)``."""
    rows = packed_b.numel()
    if c_in <= 0 or c_in % 32 or rows == 0 or rows % 16 or packed_w.numel() != rows * c_in:
        raise ValueError(f"not a packed 1 x 1 convolution of {c_in} input channels: {packed_w.numel()} weights, "
                         f"{rows} biases")
    w = packed_w.view(rows // 16, c_in // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(rows, c_in, 1, 1)
    return w.contiguous(), packed_b.clone()


class BasicEncoder:
    """The packed parameters of a ``BasicEncoder`` (extractor.py:75-141;
    ``DroidNet.fnet`` with ``norm="instance"``, ``.cnet`` with ``norm="none"``),
    packed once: ``stem`` (``pack_stem7x7``), ``head`` (``pack_conv1x1``, 128 or
    256 rows) and ``convs``, per residual block ``layerL.B`` the launches
    ``conv1`` and ``conv2`` as ``(w3, w1, bias, rows3, rows1)``: ``w3`` the 3 x 3
    convolution (``pack_conv3x3_wide``), ``w1`` the block's 1 x 1 downsample
    (``pack_conv1x1``; ``layer2.0`` and ``layer3.0`` only, else None), ``bias``
    float32 [rows3 + rows1]."""

    def __init__(self, norm, stem, convs, head):
        self.norm, self.stem, self.convs, self.head = norm, stem, convs, head
        self.out_dim = BE_OUT[norm]
        # (w3, rows3, w1, rows1, bias) of each launch as wgsr_droid_be_conv takes them
        self.args = {k: (w3.data_ptr(), rows3, _lib.ptr(w1), rows1, bias.data_ptr())
                     for k, (w3, w1, bias, rows3, rows1) in convs.items()}

    @classmethod
    def from_state_dict(cls, sd, prefix="fnet.", norm="instance", device=None):
        """From the reference module's ``state_dict`` entries ``<prefix>conv1``,
        ``layer1.0.conv1`` .. ``layer3.1.conv2``, ``layer2.0.downsample.0``,
        ``layer3.0.downsample.0`` and ``conv2`` (``.weight`` / ``.bias`` each;
        ``DroidNet``'s prefixes are "fnet." and "cnet.", the module's own "")."""
        if norm not in BE_OUT:
            raise ValueError(f"norm must be 'instance' (fnet) or 'none' (cnet): got {norm!r} (batch and group norm are "
                             "not built)")
        get = lambda k: (sd[f"{prefix}{k}.weight"], sd[f"{prefix}{k}.bias"])  # noqa: E731
        device = torch.device(device) if device is not None else get("conv1")[0].device
        _stem_check(*get("conv1"))
        names, c_in = ["conv1"], BE_DIMS[0]
        for name in BE_LAYERS:
            c_out = BE_DIMS[int(name[5]) - 1]
            for k, ci in (("conv1", c_in), ("conv2", c_out)) + ((("downsample.0", c_in),) if c_out != c_in else ()):
                w, b = get(f"{name}.{k}")
                shape = (c_out, ci) + ((1, 1) if k == "downsample.0" else (3, 3))
                if tuple(w.shape) != shape or b.numel() != c_out:
                    raise ValueError(f"{name}.{k} must be weight {shape} and bias ({c_out}): got {tuple(w.shape)} and "
                                     f"{tuple(b.shape)}")
                names.append(f"{name}.{k}")
            c_in = c_out
        w, b = get("conv2")
        if tuple(w.shape) != (BE_OUT[norm], BE_DIMS[2], 1, 1) or b.numel() != BE_OUT[norm]:
            raise ValueError(f"conv2 must be weight ({BE_OUT[norm]}, {BE_DIMS[2]}, 1, 1) with norm = {norm!r}: got "
                             f"{tuple(w.shape)}")
        names.append("conv2")

        def make():  # (one entry of the cache for the whole encoder)
            convs = {}
            for name in names[1:-1]:
                if name.endswith("downsample.0"):
                    continue
                w, b = get(name)
                w3, b3 = _pack_layout(w.detach().to(device, torch.float16),
                                      b.detach().to(device, torch.float32).reshape(-1))
                down = name.replace("conv1", "downsample.0")
                if down != name and down in names:
                    w1, b1 = _conv1x1_layout(*get(down), device)
                    convs[name] = (w3, w1, torch.cat([b3, b1]), w.size(0), w.size(0))
                else:
                    convs[name] = (w3, None, b3, w.size(0), 0)
            return cls(norm, _stem_layout(*get("conv1"), device), convs, _conv1x1_layout(*get("conv2"), device))
        return _cached(tuple(t for k in names for t in get(k)), (device, "basic_encoder", norm), make)


def be_sizes(H, W):
    """The map sizes of the three levels: ((ceil(H / 2), ceil(W / 2)), (.. / 4), (.. / 8))"""
    out = []
    for _ in range(3):
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W))
    return tuple(out)


def _be_check_size(norm, H, W):
    h1, w1 = be_sizes(H, W)[0]
    if H <= 0 or W <= 0 or h1 * w1 >= 1 << 20:
        raise ValueError(f"images of {H} x {W}: the map of {h1} x {w1} must hold between 1 and 2^20 - 1 pixels")
    h3, w3 = be_sizes(H, W)[2]
    if norm == "instance" and h3 * w3 == 1:
        raise ValueError(f"images of {H} x {W}: the last map is one pixel, which an instance norm cannot normalise "
                         "(torch raises as well)")


class BasicEncoderWorkspace:
    """Every buffer a ``feature_encoder`` / ``context_encoder`` call on ``n``
    images of ``H`` x ``W`` writes besides its result, so that a captured call has
    stable addresses: the raw maps ``R0`` .. ``R12`` (``R5`` / ``Rd5`` and ``R9`` /
    ``Rd9`` the halves of the stacked stride-2 launches' outputs), the block
    outputs ``X0``, ``X1``, ``X3``, ``X5`` and, with ``norm="instance"``, the
    statistics ``S0`` .. ``S12`` (float32 [n, C, 2]: mean, rstd) with the partial
    sums they are merged from."""

    def __init__(self, n, H, W, norm, device):
        if norm not in BE_OUT:
            raise ValueError(f"norm must be 'instance' or 'none': got {norm!r}")
        _be_check_size(norm, H, W)
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.n, self.H, self.W, self.norm, self.device = n, H, W, norm, device
        sizes = be_sizes(H, W)
        half = lambda c, s: torch.empty(n, c, *s, dtype=torch.float16, device=self.device)  # noqa: E731
        t = self.maps = {}
        for k in range(13):
            level = 0 if k < 5 else 1 if k < 9 else 2
            t[f"R{k}"] = half(BE_DIMS[level] * (2 if k in (5, 9) else 1), sizes[level])
        for k, level in ((0, 0), (1, 0), (3, 1), (5, 2)):
            t[f"X{k}"] = half(BE_DIMS[level], sizes[level])
        self.stats, self.part = {}, None
        if norm == "instance":
            L = _lib.load()
            most = 0
            for k in range(13):
                rows, s = t[f"R{k}"].size(1), t[f"R{k}"].shape[2:]
                self.stats[f"S{k}"] = torch.empty(n, rows, 2, dtype=torch.float32, device=self.device)
                most = max(most, rows * L.wgsr_droid_be_parts(s[0], s[1], 2 if k in (5, 9) else 1))
            self.part = torch.empty(n * most * 3, dtype=torch.float32, device=self.device)
        # what the launches take of these buffers, looked up once: a source as (map, frame stride, statistics,
        # frame stride), the output and the statistics launch (statistics, n, rows, partials) of each raw map
        self.src, self.dst, self.fin = {}, {}, {}
        for name, r in self.named().items():
            if name[0] == "S":
                continue
            st = self.named().get("S" + name[1:]) if name[0] == "R" else None
            self.src[name] = (r.data_ptr(), r.stride(0), _lib.ptr(st), st.stride(0) if st is not None else 0)
        for name, r in t.items():
            if name[0] == "R":
                self.dst[name] = r.data_ptr()
                if norm == "instance":
                    parts = L.wgsr_droid_be_parts(r.size(2), r.size(3), 2 if name in ("R5", "R9") else 1)
                    self.fin[name] = (self.stats["S" + name[1:]].data_ptr(), n, r.size(1), parts)

    def named(self):
        """name -> tensor: the raw maps (the stacked ones as their halves), block outputs and statistics; views"""
        out = {}
        for src, pre in ((self.maps, "R"), (self.stats, "S")):
            for name, t in src.items():
                if name in ("R5", "R9", "S5", "S9"):
                    c = t.size(1) // 2
                    out[name], out[f"{pre}d{name[1:]}"] = t[:, :c], t[:, c:]
                else:
                    out[name] = t
        return out


def _be_params(params, norm, dev):
    if isinstance(params, BasicEncoder):
        if params.norm != norm:
            raise ValueError(f"params were packed with norm = {params.norm!r}; this call needs {norm!r}")
        return params
    name = "fnet." if norm == "instance" else "cnet."
    prefix = name if f"{name}conv1.weight" in params else ""
    return BasicEncoder.from_state_dict(params, prefix, norm, dev)


def _be_run(who, norm, images, params, mean, std, out, workspace, return_intermediates):
    _inference_only(who, images=images)
    dev = droid_backends._device_of(images=images)
    images = _activation("images", images, 3, dev, dtypes=tuple(droid_backends._DTYPE_TAG))
    n, _, H, W = images.shape
    _be_check_size(norm, H, W)
    p = _be_params(params, norm, dev)
    if p.stem[0].device != dev:
        raise RuntimeError(f"params: expected tensors on {dev}, got {p.stem[0].device}")
    if (mean is None) != (std is None):
        raise ValueError("mean and std come together")
    if mean is not None:
        mean, std = (torch.as_tensor(v, dtype=torch.float32, device=dev).reshape(-1).contiguous() for v in (mean, std))
        if mean.numel() != 3 or std.numel() != 3:
            raise ValueError("mean and std must hold 3 values each")
    ws = workspace
    if ws is None:
        ws = BasicEncoderWorkspace(n, H, W, norm, dev)
    elif (ws.n, ws.H, ws.W, ws.norm, ws.device) != (n, H, W, norm, dev):
        raise ValueError(f"workspace: made for {ws.n} images of {ws.H} x {ws.W}, norm {ws.norm!r}, on {ws.device}; "
                         f"got {n} of {H} x {W}, {norm!r}, on {dev}")
    sizes = be_sizes(H, W)
    shape = (n, BE_DIMS[2]) + sizes[2]
    if norm == "instance":
        outs = (_out_buffer("out", out, shape, torch.float16, dev),)
    else:
        if out is not None and len(out) != 2:
            raise ValueError("out must hold the two buffers (net, inp)")
        outs = tuple(_out_buffer(k, out[i] if out else None, shape, torch.float16, dev) for i, k in
                     enumerate(("net", "inp")))
    if n == 0:
        res = outs[0] if norm == "instance" else outs
        return (res, ws.named()) if return_intermediates else res
    L = _lib.load()
    stream = _lib.stream_handle(dev)
    inst = norm == "instance"
    part = _lib.ptr(ws.part)
    none = (None, 0, None, 0)
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_be_stem(images.data_ptr(), droid_backends._DTYPE_TAG[images.dtype], _lib.ptr(mean),
                                        _lib.ptr(std), p.stem[0].data_ptr(), p.stem[1].data_ptr(), ws.dst["R0"], part,
                                        n, H, W, stream))
        if inst:
            _lib.check(L.wgsr_droid_be_stats(part, *ws.fin["R0"], stream))
        for name, main, second, side, c_in, stride, dst in BE_LAUNCHES:
            hi, wi = sizes[BE_DIMS.index(c_in)]
            _lib.check(L.wgsr_droid_be_conv(*ws.src[main], *(ws.src[second] if second else none),
                                            ws.src[side][0] if side else None, c_in, stride, *p.args[name], 0,
                                            ws.dst[dst], None, part, n, hi, wi, stream))
            if inst:
                _lib.check(L.wgsr_droid_be_stats(part, *ws.fin[dst], stream))
        _lib.check(L.wgsr_droid_be_conv(*ws.src["R12"], *ws.src["X5"], None, BE_DIMS[2], 1, None, 0,
                                        p.head[0].data_ptr(), p.out_dim, p.head[1].data_ptr(), 0 if inst else 1,
                                        outs[0].data_ptr(), None if inst else outs[1].data_ptr(), None, n, *sizes[2],
                                        stream))
    res = outs[0] if inst else outs
    return (res, ws.named()) if return_intermediates else res


def feature_encoder(images, params, mean=None, std=None, out=None, workspace=None, return_intermediates=False):
    """``DroidNet.fnet`` (droid_net.py:159; the ``BasicEncoder`` of extractor.py:
    75-141 with an instance norm): ``images`` [n, 3, H, W] float32 or float16 (a
    leading batch dimension of 1 is accepted and dropped) -> float16 [n, 128,
    ceil(H / 8), ceil(W / 8)].  ``params``: a ``BasicEncoder`` or the
    ``state_dict`` of ``DroidNet`` / of the module.  With ``mean`` / ``std`` (3
    values each) the stem reads ``(images - mean) / std``, computed in float32
    and rounded to float16 once, in place of ``inputs.sub_(MEAN).div_(STDV)``
    (motion_filter.py:61-62).  14 convolution launches and, for the instance
    norm, one small launch per raw map that merges its statistics; every
    convolution writes its raw output once, and the norm, the ReLU and the
    residual sum are applied as the next launch stages its tile (fp32, one
    rounding), so that no launch only normalises, activates or adds.  No
    allocation with ``workspace`` (a ``BasicEncoderWorkspace``) and ``out``, no
    synchronisation, no host read: capturable in a graph.  Two runs give the same
    bits, and an image's result does not depend on the others of the batch.
    ``return_intermediates``: ``(out, {name: tensor})`` with the raw maps, block
    outputs and statistics (``BasicEncoderWorkspace.named``)."""
    return _be_run("feature_encoder", "instance", images, params, mean, std, out, workspace, return_intermediates)


def context_encoder(images, params, mean=None, std=None, out=None, workspace=None, return_intermediates=False):
    """``DroidNet.cnet`` with the split of motion_filter.py:42-43: ``(net, inp)
    = (tanh(x[:, :128]), relu(x[:, 128:]))`` of the 256-row head, two float16 [n,
    128, ceil(H / 8), ceil(W / 8)] tensors written by the head's launch.  As
    ``feature_encoder`` without a norm: no statistics are computed or read.
    ``out``: the pair of buffers."""
    return _be_run("context_encoder", "none", images, params, mean, std, out, workspace, return_intermediates)


# ---------------------------------------------------------------------------
# The DINO-consistency filter of the metric depth prior (csrc/droid_mono_filter.hip)
# ---------------------------------------------------------------------------
DINO_PATCH = 14  # the DINO maps are [H // 14, W // 14, C]
MONO_FILTER_STATUS = {1: "an entry of jj is outside [0, N) (WGSR_MONO_FILTER_BAD_JJ)"}


def mono_filter_workspace_bytes(n_ref, H, W):
    """Bytes of device scratch ``filter_mono_depth`` needs for ``n_ref`` reference
    frames of H x W pixels: the winner words and the Gram matrices."""
    nbytes = _lib.load().wgsr_droid_mono_filter_workspace_bytes(n_ref, H, W, H // DINO_PATCH, W // DINO_PATCH)
    if nbytes < 0:
        _lib.check(1)  # WGSR_EINVAL: raises with the library's message for the refused sizes
    return nbytes


def filter_mono_depth(poses, mono_disps_up, mono_mask_up, intrinsics, dino_feats, idx, jj, sim_thresh=0.9,
                      err_thresh=0.02, return_counts=False, check=True, workspace=None):
    """``DepthVideo.filter_high_err_mono_depth`` (depth_video.py:281-349) on the
    video buffers: clears the pixels of ``mono_mask_up[idx]`` whose metric depth
    disagrees with the depth reprojected from the frames ``jj``, a reprojected
    pixel counting only where the DINO features of the two pixels match.

    ``poses`` [N, 7], ``mono_disps_up`` [N, H, W] float32 and ``mono_mask_up``
    [N, H, W] bool (row ``idx`` is updated in place) on the device;
    ``intrinsics``: frame 0's (fx, fy, cx, cy) at 1/8 scale, multiplied by
    ``down_scale`` = 8 inside as the reference does; ``dino_feats`` [N, H // 14,
    W // 14, C] float32 on any device -- the reference keeps them on the host,
    and they may stay there: the rows ``idx`` and ``jj`` are then copied over,
    about 1.5 MB a frame; ``jj`` the 1-D list of reference frames, which the
    caller takes from the graph as ``graph.jj[graph.ii == idx]``.  (The
    reference's loop that would pad ``jj`` up to
    ``nb_ref_frame_metric_depth_filtering`` frames discards the result of its
    ``torch.cat``: it does nothing, and nothing is padded here.)

    For each j of ``jj`` and each pixel (x, y) of frame j: the point ((x - cx) /
    fx, (y - cy) / fy, 1) with disparity D = ``mono_disps_up[j, y, x]`` goes
    through pose[idx] pose[j]^-1; a depth Z < 0.1 is replaced by 1 (the
    reference's ``proj``); the target is the projection rounded half to even,
    valid inside the image with d = D / Z > 0.  The candidate is matched when
    the cosine of frame j's DINO feature at (x, y) and frame idx's at the target,
    both sampled bilinearly (``align_corners=False``) from the cell maps,
    exceeds ``sim_thresh``.  Among the matched candidates of one (j, target) the
    one with the largest source index y W + x wins -- what the reference's
    scatter yields in order on one CPU thread, and here the defined rule where
    the reference's ``index_put`` is nondeterministic on a GPU.  With w the
    winner's d, ``|1 / w - 1 / mono_disps_up[idx, target]| w < err_thresh``
    (a zero disparity: inf) adds one to the target's accurate count, else to
    its inaccurate count: once per (j, target).  The mask is cleared where
    accurate <= 1, inaccurate > 0 and the disparity of idx is positive.  An
    empty ``jj`` changes nothing; a j listed twice counts twice.

    No full-resolution feature map is formed: the cosines are 16 + 20 entries of
    the cell Gram matrices (fp32 MFMA), exact up to the order of the fp32 sums.
    Four launches, no host read with the features on the device and
    ``check=False``: the call can be captured in a graph (``jj`` then has to be a
    device tensor already), and two calls give the same bits.  ``check`` reads
    the kernel's status word back and raises ``RuntimeError`` for an entry of
    ``jj`` outside [0, N) (nothing was written); ``idx`` is always checked.
    ``return_counts``: ``(accurate, inaccurate)``, int32 [H, W].  ``workspace``: a
    uint8 device tensor of at least ``mono_filter_workspace_bytes(len(jj), H, W)``
    bytes to use as scratch, e.g. one buffer the tracker keeps across keyframes;
    without it the scratch is allocated per call."""
    who = "filter_mono_depth"
    _inference_only(who, poses=poses, mono_disps_up=mono_disps_up, dino_feats=dino_feats)
    if poses.dim() != 2 or poses.size(1) != 7 or poses.dtype != torch.float32:
        raise RuntimeError("poses must be a float32 tensor of dimensions (N, 7)")
    if mono_disps_up.dim() != 3 or mono_disps_up.dtype != torch.float32:
        raise RuntimeError("mono_disps_up must be a float32 tensor of dimensions (N, H, W)")
    if mono_mask_up.dtype != torch.bool or mono_mask_up.shape != mono_disps_up.shape:
        raise RuntimeError(f"mono_mask_up must be a bool tensor of mono_disps_up's dimensions "
                           f"{tuple(mono_disps_up.shape)}: got {mono_mask_up.dtype} {tuple(mono_mask_up.shape)}")
    H, W = mono_disps_up.size(1), mono_disps_up.size(2)
    hd, wd = H // DINO_PATCH, W // DINO_PATCH
    if dino_feats.dim() != 4 or dino_feats.dtype != torch.float32:
        raise RuntimeError("dino_feats must be a float32 tensor of dimensions (N, H // 14, W // 14, C)")
    if hd < 1 or wd < 1 or tuple(dino_feats.shape[1:3]) != (hd, wd):
        raise ValueError(f"dino_feats must be (N, {hd}, {wd}, C) for frames of {H} x {W}: got "
                         f"{tuple(dino_feats.shape)}")
    C = dino_feats.size(3)
    if C == 0 or C % 4 != 0:
        raise ValueError(f"dino_feats: the channel count C = {C} must be a positive multiple of 4")
    intrinsics = torch.as_tensor(intrinsics)
    if intrinsics.numel() != 4:
        raise RuntimeError("intrinsics must have 4 elements (fx, fy, cx, cy)")
    jj = torch.as_tensor(jj)
    if jj.numel() == 0:  # (an empty list comes out as a float tensor)
        jj = jj.to(torch.int64)
    if jj.dim() != 1 or jj.dtype.is_floating_point or jj.dtype == torch.bool:
        raise RuntimeError("jj must be a 1-D tensor (or list) of frame indices")
    N = min(poses.size(0), mono_disps_up.size(0), dino_feats.size(0))
    idx = int(idx)
    if not 0 <= idx < N:
        raise RuntimeError(f"idx = {idx} must index frames [0, {N})")
    droid_backends._contiguous(poses=poses, mono_disps_up=mono_disps_up, mono_mask_up=mono_mask_up)
    dev = droid_backends._device_of(poses=poses, mono_disps_up=mono_disps_up, mono_mask_up=mono_mask_up)
    packed = dino_feats.device != dev
    if packed and dino_feats.device.type == "cuda":
        raise RuntimeError(f"dino_feats: expected a tensor on {dev} or on the host, got {dino_feats.device}")
    if packed or (check and jj.device.type == "cpu"):
        # the features are gathered by jj on the host (or jj is there already): bounded here
        jj_host = jj.to("cpu", torch.int64)
        if jj_host.numel() and (int(jj_host.min()) < 0 or int(jj_host.max()) >= N):
            raise RuntimeError(f"{who}: jj must index frames [0, {N}): got values in [{int(jj_host.min())}, "
                               f"{int(jj_host.max())}]; nothing was written")
    E = jj.numel()
    counts = None
    if return_counts:  # (every element is written by the call)
        make = torch.empty if E else torch.zeros
        counts = (make(H, W, dtype=torch.int32, device=dev), make(H, W, dtype=torch.int32, device=dev))
    if E == 0:
        return counts
    if packed:
        rows = torch.cat([torch.tensor([idx], dtype=torch.int64), jj_host])
        feats = dino_feats.detach()[rows].to(dev).contiguous()
    else:
        feats = dino_feats.detach()
        droid_backends._contiguous(dino_feats=feats)
    jj = jj.to(dev, torch.int64).contiguous()
    intrinsics = intrinsics.detach().to(dev, torch.float32).reshape(-1).contiguous()
    L = _lib.load()
    nbytes = mono_filter_workspace_bytes(E, H, W)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif (workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous()
          or workspace.numel() < nbytes or workspace.data_ptr() % 16):
        raise RuntimeError(f"workspace must be a contiguous, 16-byte aligned uint8 tensor of at least {nbytes} bytes "
                           f"on {dev} (mono_filter_workspace_bytes)")
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_droid_mono_filter(poses.data_ptr(), mono_disps_up.data_ptr(), mono_mask_up.data_ptr(),
                                            intrinsics.data_ptr(), feats.data_ptr(), int(packed), jj.data_ptr(), E, idx,
                                            N, H, W, hd, wd, C, float(sim_thresh), float(err_thresh),
                                            _lib.ptr(counts[0]) if counts else None,
                                            _lib.ptr(counts[1]) if counts else None, workspace.data_ptr(),
                                            workspace.numel(),
                                            status.data_ptr(), _lib.stream_handle(dev)))
    if check:
        _raise_status(who, status, MONO_FILTER_STATUS)
    return counts
