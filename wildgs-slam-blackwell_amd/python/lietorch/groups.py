"""The group classes of the ``lietorch`` drop-in (see the package docstring).

Every kernel-backed operation is one launch of ``wgsr_lie_se3``: the batch
shapes of the two operands are broadcast, and an operand that is constant over
trailing dimensions of the result (a pose against a [.., H, W, 4] point map)
is passed as it is with its repeat count; any other broadcast pattern is
expanded first."""
from __future__ import annotations

import math

import torch

from wgsr import _lib

# WGSR_LIE_* (include/wgsr.h)
_EXP, _LOG, _INV, _MUL, _ACT3, _ACT4, _MATRIX, _ADJ, _ADJT, _RETR = range(10)


def _check_inputs(*tensors):
    """grad mode, dtype and device, before any launch; returns the device"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise NotImplementedError("lietorch on this platform is inference only: an input requires grad "
                                  "(call it under torch.no_grad())")
    dev = None
    for t in tensors:
        if t.device.type != "cuda":
            raise RuntimeError(f"lietorch: expected a HIP device tensor, got {t.device}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"lietorch: only float32 is built, got {t.dtype}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"lietorch: expected a tensor on {dev}, got {t.device}")
    return dev


def _operand(t, batch):
    """(contiguous tensor, inner) with flat result element e reading element
    e // inner of the tensor"""
    nd = len(batch)
    bs = (1,) * (nd - (t.dim() - 1)) + tuple(t.shape[:-1])
    for k in range(nd + 1):
        if any(s != 1 for s in bs[nd - k:]):
            break
        if bs[:nd - k] == tuple(batch[:nd - k]):
            return t.contiguous(), max(1, math.prod(batch[nd - k:]))
    return t.expand(tuple(batch) + (t.shape[-1],)).contiguous(), 1


def _launch(op, a, b, out_dim):
    dev = _check_inputs(*((a,) if b is None else (a, b)))
    batch = tuple(a.shape[:-1]) if b is None else torch.broadcast_shapes(a.shape[:-1], b.shape[:-1])
    out = torch.empty(tuple(batch) + (out_dim,), dtype=torch.float32, device=dev)
    n = out.numel() // out_dim
    if n == 0:
        return out
    a, inner_a = _operand(a, batch)
    pb, inner_b = None, 1
    if b is not None:
        b, inner_b = _operand(b, batch)
        pb = b.data_ptr()
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.wgsr_lie_se3(op, a.data_ptr(), inner_a, pb, inner_b, out.data_ptr(), n,
                                  _lib.stream_handle(dev)))
    return out


class LieGroup:
    group_name = None
    manifold_dim = None
    embedded_dim = None
    id_elem = None
    _built = False

    def __init__(self, data):
        if not type(self)._built:
            raise NotImplementedError(f"lietorch.{type(self).group_name} is not built on this platform "
                                      f"(only SE3 is)")
        if isinstance(data, LieGroup):
            data = data.data
        if data.shape[-1] != self.embedded_dim:
            raise ValueError(f"{self.group_name} data must have last dimension {self.embedded_dim}, "
                             f"got {tuple(data.shape)}")
        self.data = data

    def __repr__(self):
        return f"{self.group_name}: size={tuple(self.shape)}, device={self.device}, dtype={self.dtype}"

    @property
    def shape(self):
        return self.data.shape[:-1]

    @property
    def device(self):
        return self.data.device

    @property
    def dtype(self):
        return self.data.dtype

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, index):
        # an Ellipsis covers batch dimensions only: the element's own stays last
        if index is Ellipsis:
            return self.__class__(self.data)
        if isinstance(index, tuple) and any(i is Ellipsis for i in index):
            index = index + (slice(None),)
        return self.__class__(self.data[index])

    def __setitem__(self, index, item):
        self.data[index] = item.data

    def view(self, *dims):
        if len(dims) == 1 and isinstance(dims[0], (tuple, list, torch.Size)):
            dims = tuple(dims[0])
        return self.__class__(self.data.view(tuple(dims) + (self.embedded_dim,)))

    def reshape(self, *dims):
        if len(dims) == 1 and isinstance(dims[0], (tuple, list, torch.Size)):
            dims = tuple(dims[0])
        return self.__class__(self.data.reshape(tuple(dims) + (self.embedded_dim,)))

    def to(self, *args, **kwargs):
        return self.__class__(self.data.to(*args, **kwargs))

    def cpu(self):
        return self.__class__(self.data.cpu())

    def cuda(self, *args, **kwargs):
        return self.__class__(self.data.cuda(*args, **kwargs))

    def float(self):
        return self.__class__(self.data.float())

    def double(self):
        return self.__class__(self.data.double())

    def clone(self):
        return self.__class__(self.data.clone())

    def detach(self):
        return self.__class__(self.data.detach())

    def vec(self):
        return self.data

    def tensor(self):
        return self.data

    @classmethod
    def Identity(cls, *batch_shape, **kwargs):
        if len(batch_shape) == 1 and isinstance(batch_shape[0], (tuple, list, torch.Size)):
            batch_shape = tuple(batch_shape[0])
        kwargs.setdefault("dtype", torch.float32)
        e = torch.tensor(cls.id_elem, **kwargs)
        return cls(e.repeat(tuple(batch_shape) + (1,)))

    @classmethod
    def IdentityLike(cls, G):
        return cls.Identity(G.shape, device=G.data.device, dtype=G.dtype)


class SE3(LieGroup):
    group_name = "SE3"
    manifold_dim = 6
    embedded_dim = 7
    id_elem = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    _built = True

    @classmethod
    def exp(cls, x):
        """x [..., 6] = (tau, phi)"""
        return cls(_launch(_EXP, x, None, 7))

    def log(self):
        return _launch(_LOG, self.data, None, 6)

    def inv(self):
        return SE3(_launch(_INV, self.data, None, 7))

    def matrix(self):
        """[..., 4, 4]"""
        return _launch(_MATRIX, self.data, None, 16).view(tuple(self.shape) + (4, 4))

    def translation(self):
        """[..., 4] = (tx, ty, tz, 1): the group's action on (0, 0, 0, 1)"""
        return torch.cat([self.data[..., :3], torch.ones_like(self.data[..., :1])], dim=-1)

    def mul(self, other):
        return SE3(_launch(_MUL, self.data, other.data, 7))

    def act(self, p):
        """p [..., 3]: R p + t; p [..., 4] = (X, Y, Z, w): (R XYZ + w t, w)"""
        if p.shape[-1] == 3:
            return _launch(_ACT3, self.data, p, 3)
        if p.shape[-1] == 4:
            return _launch(_ACT4, self.data, p, 4)
        raise ValueError(f"SE3 acts on points with last dimension 3 or 4, got {tuple(p.shape)}")

    def __mul__(self, other):
        if isinstance(other, LieGroup):
            if not isinstance(other, SE3):
                raise NotImplementedError(f"SE3 * {type(other).group_name} is not built")
            return self.mul(other)
        if isinstance(other, torch.Tensor):
            return self.act(other)
        return NotImplemented

    def retr(self, a):
        """exp(a) * self"""
        return SE3(_launch(_RETR, self.data, a, 7))

    def adj(self, a):
        """Adj a, with Adj = [[R, [t]x R], [0, R]]"""
        return _launch(_ADJ, self.data, a, 6)

    def adjT(self, a):
        """Adj^T a"""
        return _launch(_ADJT, self.data, a, 6)


class SO3(LieGroup):
    group_name = "SO3"
    manifold_dim = 3
    embedded_dim = 4
    id_elem = [0.0, 0.0, 0.0, 1.0]


class RxSO3(LieGroup):
    group_name = "RxSO3"
    manifold_dim = 4
    embedded_dim = 5
    id_elem = [0.0, 0.0, 0.0, 1.0, 1.0]


class Sim3(LieGroup):
    group_name = "Sim3"
    manifold_dim = 7
    embedded_dim = 8
    id_elem = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]


def _batch_dim(group, dim):
    nd = group.data.dim() - 1
    return dim + nd if dim < 0 else dim


def cat(group_list, dim):
    """concatenate along batch dimension ``dim``"""
    g = group_list[0]
    return g.__class__(torch.cat([x.data for x in group_list], dim=_batch_dim(g, dim)))


def stack(group_list, dim):
    """stack along a new batch dimension ``dim``"""
    g = group_list[0]
    nd = g.data.dim()  # (a new batch dimension may follow the last one)
    return g.__class__(torch.stack([x.data for x in group_list], dim=dim + nd if dim < 0 else dim))
