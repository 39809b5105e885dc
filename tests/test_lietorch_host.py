"""CPU tests of the ``lietorch`` drop-in's surface (python/lietorch): what the
reference's tracker imports and the plumbing it does on group objects --
construction, every indexing form it uses, ``Identity``, ``cat`` / ``stack``,
in-place writes through ``.data`` -- plus the errors of what is not built.
The group operations themselves run on the GPU (tests/test_gpu_lie.py)."""
import pytest
import torch


def _poses(*batch):
    g = torch.Generator().manual_seed(0)
    d = torch.randn(*batch, 7, generator=g)
    d[..., 3:] /= d[..., 3:].norm(dim=-1, keepdim=True)
    return d


def test_import_surface():
    import lietorch
    from lietorch import SE3, Sim3  # noqa: F401  (projective_ops.py:18)
    from lietorch import SO3, RxSO3  # noqa: F401
    assert callable(lietorch.cat) and callable(lietorch.stack)
    assert SE3.manifold_dim == 6 and SE3.embedded_dim == 7
    G = SE3(_poses(1, 5))
    assert isinstance(G, SE3) and not isinstance(G, Sim3)
    assert tuple(G.shape) == (1, 5) and G.device == G.data.device and G.dtype == torch.float32
    for name in ("exp", "log", "inv", "matrix", "vec", "translation", "retr", "adj", "adjT", "view", "to", "cpu",
                 "cuda", "clone", "detach", "Identity"):
        assert hasattr(SE3, name), name


def test_indexing_forms_of_the_reference():
    from lietorch import SE3
    data = _poses(1, 6)
    G = SE3(data)
    ii = torch.tensor([0, 2, 5, 2])
    assert tuple(G[:, ii].shape) == (1, 4) and torch.equal(G[:, ii].data, data[:, ii])
    assert tuple(G[None].shape) == (1, 1, 6)
    assert tuple(G[:, :, None, None].shape) == (1, 6, 1, 1)
    assert tuple(G[:, :, None, None].data.shape) == (1, 6, 1, 1, 7)
    assert tuple(G[:, :, None, None, None].shape) == (1, 6, 1, 1, 1)
    assert tuple(G[..., None].shape) == (1, 6, 1) and tuple(G[..., None].data.shape) == (1, 6, 1, 7)
    assert torch.equal(G[..., None].data[:, :, 0], data)
    assert tuple(G[...].shape) == (1, 6)
    P = SE3(data[0])  # trajectory_filler.py:58-66: Ps[t1]
    t1 = torch.tensor([1, 1, 3])
    assert tuple(P[t1].shape) == (3,) and torch.equal(P[t1].data, data[0][t1])
    assert tuple(P[2].shape) == () and tuple(P[1:4].shape) == (3,)
    assert tuple(G.view(6).shape) == (6,) and tuple(G.view(2, 3).shape) == (2, 3)
    assert G.view(2, 3).data.shape == (2, 3, 7)


def test_plumbing_keeps_the_class_and_the_data():
    from lietorch import SE3
    G = SE3(_poses(4))
    for H in (G.clone(), G.detach(), G.cpu(), G.to("cpu"), G.to(torch.float64), SE3(G)):
        assert isinstance(H, SE3) and tuple(H.shape) == (4,)
    assert G.to(torch.float64).dtype == torch.float64
    assert G.clone().data.data_ptr() != G.data.data_ptr()
    assert torch.equal(G.vec(), G.data)
    tr = G.translation()
    assert tr.shape == (4, 4) and torch.equal(tr[:, :3], G.data[:, :3]) and torch.all(tr[:, 3] == 1)


def test_identity_cat_stack():
    import lietorch
    from lietorch import SE3
    Id = SE3.Identity(1,)  # motion_filter.py:55
    assert torch.equal(Id.data.squeeze(), torch.tensor([0.0, 0, 0, 0, 0, 0, 1]))
    I2 = SE3.Identity(2, 3, dtype=torch.float64)
    assert tuple(I2.shape) == (2, 3) and I2.dtype == torch.float64
    assert torch.all(I2.data[..., 6] == 1) and torch.all(I2.data[..., :6] == 0)
    I2.data[0, 0, 0] = 5.0  # writable, not an expanded view
    assert I2.data[1, 0, 0] == 0
    a, b = SE3(_poses(2)), SE3(_poses(3))
    c = lietorch.cat([a, b], dim=0)  # trajectory_filler.py:139
    assert isinstance(c, SE3) and tuple(c.shape) == (5,) and torch.equal(c.data[2:], b.data)
    s = lietorch.stack([a, a], dim=0)
    assert tuple(s.shape) == (2, 2) and tuple(s.data.shape) == (2, 2, 7)
    s = lietorch.stack([a, a], dim=-1)
    assert tuple(s.shape) == (2, 2) and torch.equal(s.data[:, 1], a.data)


def test_in_place_assignment_through_data():
    from lietorch import SE3
    G = SE3(_poses(1, 4))
    ii, jj = torch.tensor([0, 1, 2, 3]), torch.tensor([1, 1, 0, 3])
    stereo = torch.as_tensor([-0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    before = G.data.clone()
    G.data[:, ii == jj] = stereo  # projective_ops.py:119
    assert torch.equal(G.data[0, 1], stereo) and torch.equal(G.data[0, 3], stereo)
    assert torch.equal(G.data[0, 0], before[0, 0]) and torch.equal(G.data[0, 2], before[0, 2])


@pytest.mark.parametrize("name", ["Sim3", "SO3", "RxSO3"])
def test_groups_not_built_raise_by_name(name):
    import lietorch
    cls = getattr(lietorch, name)
    with pytest.raises(NotImplementedError, match=name):
        cls(torch.zeros(2, cls.embedded_dim))
    with pytest.raises(NotImplementedError, match=name):
        cls.Identity(1)


def test_host_tensors_are_rejected_before_any_launch():
    from lietorch import SE3
    G = SE3(_poses(3))
    calls = [G.inv, G.log, G.matrix, lambda: G * G, lambda: G * torch.zeros(3, 3), lambda: G * torch.zeros(3, 4),
             lambda: SE3.exp(torch.zeros(3, 6)), lambda: G.retr(torch.zeros(3, 6)),
             lambda: G.adj(torch.zeros(3, 6)), lambda: G.adjT(torch.zeros(3, 6))]
    for f in calls:
        with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
            f()


def test_inputs_that_require_grad_raise():
    from lietorch import SE3
    G = SE3(_poses(3).requires_grad_())
    with pytest.raises(NotImplementedError, match="inference only"):
        G.inv()
    with pytest.raises(NotImplementedError, match="inference only"):
        SE3(_poses(3)) * torch.zeros(3, 4, requires_grad=True)
    with torch.no_grad():  # grad mode off: the device check is next
        with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
            G.inv()


def test_frontend_reproject_validates_before_any_launch():
    from wgsr import frontend
    poses, disps, intr = _poses(3), torch.ones(3, 4, 5), torch.ones(3, 4)
    ii = torch.tensor([0, 1])
    with pytest.raises(RuntimeError, match="expected a HIP device tensor"):
        frontend.reproject(poses, disps, intr, ii, ii)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        frontend.reproject(poses, disps.transpose(1, 2), intr, ii, ii)
